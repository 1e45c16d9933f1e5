/*
 * gnuais_hip.h -- C ABI of the MI355X (gfx950) batch AIS receive chain.
 *
 * This is the drop-in boundary for gnuais's per-sample hot path.  Every entry
 * point cites the reference interface it stands in for (paths relative to the
 * gnuais tree).  Plain C: opaque handle, plain pointers and sizes, int status.
 * libgnuais_hip.so is built by gnuais_amd/csrc/Makefile with hipcc for gfx950;
 * there is no CPU fallback -- every call fails with GNUAIS_E_HIP when no HIP
 * device is usable.
 *
 * One batch = N independent receivers (one per interleaved channel) that the
 * reference would create with N calls of init_receiver() (src/receiver.c:52-74)
 * and drive with N calls of receiver_run() per buffer (src/ais.c:237-247).
 */
#ifndef GNUAIS_HIP_H
#define GNUAIS_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNUAIS_OK          0
#define GNUAIS_E_ARG      -1   /* bad argument                                   */
#define GNUAIS_E_HIP      -2   /* HIP runtime / device error (see last_error)    */
#define GNUAIS_E_OVERFLOW -3   /* frame ring overflowed; oldest results kept     */
#define GNUAIS_E_STATE    -4   /* call sequence error                            */

#define GNUAIS_MAX_TAPS 1023   /* src/filter.h:28 BufferLen 1024 (len < BufferLen) */

/* One CRC-valid HDLC frame = what src/protodec.c:1100-1104 hands to
 * protodec_getdata(): `nbits` = bufferlen, payload = the bits of d->rbuffer
 * packed MSB first (AIS bit x = payload[x/8] >> (7 - x%8) & 1).  64 bytes. */
typedef struct gnuais_frame {
	uint32_t channel;      /* interleaved channel index (receiver ch_ofs)      */
	uint32_t end_bit;      /* bits fed to the deframer since reset before the
	                          bit that closed the frame, low 32 bits (orders
	                          frames in time together with flags[5:1]) */
	uint8_t  payload[53];  /* nbits/8 bytes used, rest zero                     */
	uint8_t  flags;        /* bit0: CRC ok (always set for delivered frames);
	                          bits 5:1 = bits 36:32 of end_bit: the 37-bit stamp
	                          wraps after 165 days of 9600 bit/s;
	                          bit 6 (GNUAIS_FRAME_REPAIRED): the frame failed the
	                          CRC as received and was repaired (gnuais_batch_repair) */
	uint16_t nbits;        /* bufferpos - 22, src/protodec.c:1096               */
} gnuais_frame;
#define GNUAIS_FRAME_REPAIRED 0x40   /* gnuais_frame.flags: repaired by gnuais_batch_repair / gnuais_repair_candidate */
/* The 37-bit stamp across its wrap.  A channel's bit count goes on past 2^37; the stamp is that count modulo 2^37, and
 * everything that orders frames compares stamps as plain numbers.  So for the ONE drained span of a channel whose frames
 * close on both sides of the wrap (once per 165 days of 9600 bit/s and per channel; a span whose frames all close on one
 * side is like any other):
 *   holds:  the records themselves, the stamp included -- every frame is delivered once, with the CRC state, the repair
 *           flag and the counters of any other span; the receive times (gnuais_batch_frame_times takes the distance
 *           between the count and the stamp modulo 2^37), and with them the signal records, the channel load, and the
 *           merge and order of the timed frames in gnuais_batch_drain_frames_unique / _heard;
 *   does not hold:  the order of that channel's frames inside that drain -- in gnuais_batch_drain_frames and its timed /
 *           signal forms, in the sentences and sequence digits of the drain_nmea / drain_messages / stream_nmea family,
 *           among the untimed frames of the unique drain: the frames behind the wrap come first -- and the last writer
 *           of a vessel's field groups in gnuais_batch_fold_vessels and the carried vessel table, for the vessels that
 *           channel reports on both sides (the report in front of the wrap wins).
 * The carry of the count at 2^32 (5.2 days) is an ordinary carry into flags[5:1]: nothing changes across it. */

/* One entry of the reference's position cache, struct cache_ent (src/cache.h:27-56), strings
 * inline: what the cache holds for one MMSI after the per-type decoders called cache_position /
 * cache_vesseldata / cache_vesseldatab / cache_vesseldatabb / cache_vesselname /
 * cache_vessel_persons (src/cache.c:204-384).  Fields nobody has set keep cache_get()'s
 * defaults (src/cache.c:181-196): 0 for lat/lon/draught, -1 for the other numbers, and the
 * GNUAIS_V_* bit of an unset string is clear (the reference holds NULL there).  120 bytes. */
#define GNUAIS_V_POSITION 1u    /* received_pos is set: a type 1-3 / 4 / 18 report            */
#define GNUAIS_V_DATA     2u    /* received_data is set: type 5 / 19 / 24                     */
#define GNUAIS_V_PERSONS  4u    /* received_persons_on_board is set: DAC 1 FI 40              */
#define GNUAIS_V_NAME     8u    /* name and destination hold strings                          */
#define GNUAIS_V_CALLSIGN 16u   /* callsign holds a string                                    */
#define GNUAIS_V_STATIC   32u   /* imo, shiptype, A-D, draught were written                   */
typedef struct gnuais_vessel {
	int32_t  mmsi;
	uint32_t set;              /* GNUAIS_V_* */
	float    lat, lon;
	int32_t  hdg;
	float    course, sog;
	int32_t  navstat;
	int32_t  imo;
	int32_t  shiptype, A, B, C, D;
	float    draught;
	int32_t  persons_on_board;
	char     callsign[8];      /* <= 6 characters + NUL */
	char     name[24];         /* <= 20 characters + NUL */
	char     destination[24];
} gnuais_vessel;

/* per-channel counters: src/protodec.h:58-60, bumped at src/protodec.c:1103,1107,1112,
 * read by src/ais.c:296-310 */
typedef struct gnuais_counters {
	int32_t receivedframes, lostframes, lostframes2;
} gnuais_counters;

/* per-channel carry of receiver.c's loop: src/receiver.h:38-44 */
typedef struct gnuais_pll_state {
	uint32_t pll;
	int32_t prev, lastbit;
} gnuais_pll_state;

/* per-channel deframer control state: live fields of struct demod_state_t,
 * src/protodec.h:44-57.  antallpreamble is reported saturated at 15 (only
 * "> 14" is ever tested, src/protodec.c:1036). */
typedef struct gnuais_fsm_state {
	int32_t state, nstartsign, antallpreamble, antallenner, bitstuff, last, bufferpos;
} gnuais_fsm_state;

typedef struct gnuais_batch gnuais_batch;

/* ---- lifetime: init_receiver()/free_receiver(), src/receiver.c:52-82 --------
 * taps/n_taps: filter_init(len, taps) arguments (src/filter.c:57); NULL/0 =
 *   the reference table (src/receiver.c:39-50).
 * pllinc: rx->pllinc (src/receiver.c:69); 0 = 0x10000/5.  Values above 14 426 (fewer than
 * ~4.6 samples per bit; AIS at 48 kHz has 5) are refused with GNUAIS_E_ARG: the deframer's
 * per-segment bit pack is sized for at most 16 words.
 * max_len: largest `len` a run call will be given.
 * frame_capacity: frames that can be queued between two drains; 0 = default. */
int  gnuais_batch_create(gnuais_batch **out, int device, int n_channels,
			 const float *taps, int n_taps, unsigned pllinc,
			 int max_len, int frame_capacity);
void gnuais_batch_destroy(gnuais_batch *b);
/* back to the state init_receiver()+protodec_initialize() leave (src/protodec.c:54-76) */
int  gnuais_batch_reset(gnuais_batch *b);
/* Start the batch's clocks somewhere other than zero: after the call the batch behaves as if gnuais_batch_reset() had
 * happened at chain row `rows`, with h_bits[c] bits already fed to channel c's deframer and nothing found in them
 * (h_bits: HOST uint64 [n_channels]; NULL = 0 everywhere).  This is what a restarted receiver needs to continue a saved
 * time base (save info("rows") and, per channel, a bit count at least as large as the one it had: receive times, block
 * and epoch indices and the frames' 37-bit stamps then go on from there), and what lets a test reach the carries of
 * these clocks at 2^31, 2^32 and 2^37 without days of input.
 *   Set: the row count (info("rows"), the n0 of every receive time); the deframer's bit count, low and high word, every
 *   bit of the high word stored as the deframer stores it (a frame's stamp carries the low 37 bits); and what reset
 *   latches from row 0 -- the start of the run of I/Q-type calls (gnuais_batch_frame_signal) and the origin and epochs
 *   of gnuais_batch_occupancy -- is latched from `rows` by the same code.  Nothing else changes: not the frame-start
 *   count, not the int32 counters.
 *   GNUAIS_E_ARG: rows < 0.  GNUAIS_E_STATE: a run or decode call (any gnuais_batch_run*, gnuais_batch_decode_bits,
 *   gnuais_batch_stream_nmea's runs) has been made since create / reset; or a wide stage (gnuais_batch_channeliser /
 *   _resampler) or the AFC (gnuais_batch_afc) is configured: their sample counts start at their configuration and have
 *   start-up behaviour, and what a shifted origin means for them is not defined.  The multi-device node has no such
 *   call.  Synchronises. */
int  gnuais_batch_set_clock(gnuais_batch *b, long long rows, const uint64_t *h_bits);

/* ---- hot path: receiver_run() for every channel, src/receiver.c:87-135 ------
 * d_samples: DEVICE pointer, interleaved int16 [len][n_channels] (the layout
 *   receiver_run reads with step = num_ch, src/receiver.c:102,107).
 * stream: hipStream_t (NULL = default stream).  Asynchronous; results are
 *   read after gnuais_batch_sync().  len may exceed the reference's 4096.
 *   The calls of one batch are ordered (each continues the receivers' state): use one stream for a
 *   batch; when the stream changes between two calls the previous one is synchronised first.
 *   One batch must not be driven from two host threads at once; different batches may. */
int  gnuais_batch_run(gnuais_batch *b, const int16_t *d_samples, int len, void *stream);
/* same from a HOST buffer (what src/ais.c:216-247 holds): copies H2D, runs, syncs */
int  gnuais_batch_run_host(gnuais_batch *b, const int16_t *h_samples, int len);
/* the same without waiting for the device: the samples are copied into one of two pinned staging
 * buffers (the call returns when that copy is done and `h_samples` may be reused), the transfer and
 * the chain run asynchronously on an internal stream; the next call's copy overlaps them.  Results
 * after gnuais_batch_sync().  For callers that read a file or a socket in large pieces. */
int  gnuais_batch_run_host_async(gnuais_batch *b, const int16_t *h_samples, int len);
int  gnuais_batch_sync(gnuais_batch *b);

/* ---- complex baseband in: an FM discriminator on the device in front of the chain ----------------------------
 * Not in the reference (it reads discriminator audio from a sound card); for SDR front ends and channelisers that
 * give I/Q pairs.  Per channel, a stream of int16 pairs (I, Q) at the chain's sample rate (48 kHz for the default
 * table, 192 kHz with the 144-tap table and its pllinc) becomes the int16 audio sample out[n], which enters the
 * chain exactly as if it had been passed to gnuais_batch_run().  Carried per channel: the previous pair (Ip, Qp),
 * (0, 0) after gnuais_batch_create() and gnuais_batch_reset().  Audio run calls neither read nor change it; the
 * two kinds of call may be mixed on one batch, and the carry is always the last pair an I/Q call saw.
 *
 * fp32, IEEE round-to-nearest-even at every operation, no fused multiply-add, int16 -> fp32 exact:
 *   re = (I*Ip) + (Q*Qp)      im = (Q*Ip) - (I*Qp)        each product rounded, then the sum rounded
 *   ax = |re|  ay = |im|  mx = max(ax, ay)  mn = min(ax, ay)
 *   t  = (mx == 0) ? 0 : mn / mx                         correctly rounded division
 *   s  = t*t
 *   p  = t * (A1 + s*(A3 + s*(A5 + s*(A7 + s*A9))))      in exactly this order (Abramowitz & Stegun 4.4.49)
 *   if (ay > ax) p = HALF_PI - p
 *   if (re < 0)  p = PI - p                              ordered compares: -0.0 is not < 0
 *   if (im < 0)  p = -p
 *   out = clamp(rint(p * G), -32768, 32767)              rint = round half to even
 * with the fp32 constants (bit patterns)  A1 0x3f7ff738 (0.9998660)  A3 0xbea91d04 (-0.3302995)
 *   A5 0x3e3876e2 (0.1801410)  A7 0xbdae5a36 (-0.0851330)  A9 0x3caaae5f (0.0208351)
 *   PI 0x40490fdb  HALF_PI 0x3fc90fdb  G 0x4622f983 (32768/pi).
 * out is the phase step from one pair to the next in units of pi/32768 (only +pi clips, to 32767); there is no gain.
 * The AIS deviation of +-2.4 kHz reads about +-3277 at 48 kHz and +-819 at 192 kHz.  The slicer uses only the sign of
 * the filtered value; gnuais_batch_maxval() (the level log's value) reads out in these units. */
/* d_iq = DEVICE int16 [len][n_channels][2] (I, Q), i.e. a 2N-channel interleaved stream; runs the discriminator then
 * the receive chain on its output; asynchronous as gnuais_batch_run (the discriminator runs on `stream`; a change of
 * stream between two calls synchronises the previous one first) */
int  gnuais_batch_run_iq(gnuais_batch *b, const int16_t *d_iq, int len, void *stream);
/* the same from a HOST buffer; synchronous (copy, run, sync) */
int  gnuais_batch_run_iq_host(gnuais_batch *b, const int16_t *h_iq, int len);

/* ---- wideband in: a channeliser on the device in front of the discriminator ----------------------------------
 * Not in the reference.  For SDR front ends that record both AIS channels in one complex stream (e.g. tuned to
 * 162.000 MHz: 87B at -25 kHz, 88B at +25 kHz).  Everything is integer, so the result does not depend on the order of
 * any sum.
 *   Shape: the batch's N receivers are M = N/K wide streams times K offsets (N % K == 0, 1 <= K <= 32); the input is
 *   int16 [len][M][2] (I, Q); receiver c = s*K + k is stream s tuned to offset k.  R = input rate (Hz), D = decimation,
 *   1 <= D <= 64.  n counts wide samples since the last reset or configuration, across calls.  A call's len is a
 *   multiple of D and at most D*max_len.
 *   Mixer of offset f_k (Hz, signed): period P_k = R / gcd(|f_k|, R) (f_k = 0: 1), refused if P_k > 2^20;
 *     q = (f_k * p) mod R   (exact int64, result in [0, R))
 *     C_k[p] = rnd(32767.0 * cos(2.0 * pi * q / R)),  S_k[p] = rnd(32767.0 * sin(2.0 * pi * q / R))
 *   in double (the angle as written, left to right), rnd = round half away from zero (C lround); on the host, once per
 *   configuration.
 *   Mix, p = n mod P_k (multiplication by e^{-j theta}):
 *     u = I*C + Q*S,  v = Q*C - I*S                            exact in int32
 *     mr = sat16((u + 16384) >> 15),  mi = sat16((v + 16384) >> 15)   >> arithmetic (floor), sat16 clamps to int16
 *   Filter and decimate with int16 taps h[0..T-1]: narrowband row m of the call is
 *     acc = sum_j h[j] * mr[m*D + D-1-j]   (mr before the first sample since reset / configuration = 0)
 *     out_re = sat16((acc + 16384) >> 15), the same for mi -> out_im
 *   so a call of len wide samples gives len/D rows, the last ending on the call's last sample.
 *   Taps: 1 <= T <= 1025, |h[j]| <= 32767, sum |h[j]| <= 65535 (else GNUAIS_E_ARG).  Then |u|, |v| <= 2*32768*32767
 *   < 2^31 and |acc| + 16384 <= 32768*65535 + 16384 < 2^31: every int32 order gives the same bits.
 *   Default taps (taps == NULL or n_taps == 0): a Blackman-windowed sinc, T = 16D + 1, cutoff 0.375 of the output rate:
 *     w[j] = 0.42 - 0.5 * cos(2.0 * pi * j / (T-1)) + 0.08 * cos(4.0 * pi * j / (T-1))
 *     x[j] = 0.75 * (j - 8D) / D;   s[j] = (x[j] == 0) ? 1.0 : sin(pi * x[j]) / (pi * x[j])
 *     g[j] = w[j] * s[j];   G = g[0] + g[1] + ... + g[T-1] (in that order);   h[j] = rnd(g[j] * 32768.0 / G)
 *   in double, each expression as written, left to right.  Flat to 10 kHz, -6 dB at 18 kHz and below -66 dB from
 *   26 kHz at 48 kHz out; sum |h| is about 49 000.
 * The rows (out_re, out_im) of receiver c then go through the discriminator above (a wideband call is an I/Q call for
 * its carry) and into the unchanged chain.  Carried per stream: the last T-1 wide samples; per batch: n.  Both are zero
 * after configuration and gnuais_batch_reset() (which keeps the configuration).  Audio and run_iq calls leave them
 * alone; all three kinds of call may be mixed on one batch.  A wideband call before gnuais_batch_channeliser() is
 * GNUAIS_E_ARG. */
/* configure (synchronises the device): offsets_hz[n_offsets] (n_offsets = K), taps[n_taps] or NULL / 0 = default */
int  gnuais_batch_channeliser(gnuais_batch *b, int decim, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                              const int16_t *taps, int n_taps);
/* d_wide = DEVICE int16 [len][M][2]: channeliser, discriminator and chain; asynchronous on `stream` as gnuais_batch_run_iq
 * (its narrowband I/Q goes into a batch scratch buffer [max_len][N][2]; a change of stream drains the previous one) */
int  gnuais_batch_run_wideband(gnuais_batch *b, const int16_t *d_wide, int len, void *stream);
/* the same from a HOST buffer; synchronous (copy, run, sync) */
int  gnuais_batch_run_wideband_host(gnuais_batch *b, const int16_t *h_wide, int len);
/* the channeliser only (a parity tap): d_out DEVICE int16 [len/D][N][2] (must not overlap d_wide); advances the
 * channeliser's state and nothing else.  Asynchronous on `stream`. */
int  gnuais_batch_channelise(gnuais_batch *b, const int16_t *d_wide, int len, int16_t *d_out, void *stream);
/* host only, no batch: the default taps for decim into out[cap] (*n_taps = 16*decim + 1), and offset_hz's mixer
 * table at in_rate_hz, out[cap][2] = (C, S), *period = P */
int  gnuais_channeliser_default_taps(int decim, int16_t *out, int cap, int *n_taps);
int  gnuais_channeliser_mixer_table(int in_rate_hz, int offset_hz, int16_t *out, int cap, int *period);

/* ---- wideband in at any sample rate: the channeliser at a rational ratio U/D ----------------------------------------
 * Not in the reference.  For captures whose rate is no integer multiple of the chain's (250 k = 24/125 of 48 k, 1.024 M
 * = 3/64, 2.048 M = 3/128, 2.5 M = 12/625, ...).  U = up, D = down, gcd(U, D) = 1, out rate = in rate * U / D; all
 * integer as above, shapes, offsets, formats and n as above.  Limits: 1 <= U <= 64, U < D <= 1024.
 *   Mixer: unchanged -- tables at the INPUT rate R, p = n mod P_k, the same rounding and saturation.
 *   Filter: a prototype of int16 taps h[0..T-1] at the up-sampled rate U*R.  Narrowband row m, counted since reset or
 *   configuration, ends on up-sampled tick u_m = m*D + D-1 (wide sample n sits on tick n*U):
 *     acc = sum over the j in [0, T) with (u_m - j) mod U == 0 of  h[j] * mr[(u_m - j) / U]      (mr before sample 0 = 0)
 *     out_re = sat16((acc + 16384) >> 15), the same for mi -> out_im
 *   A call takes len wide samples, len a positive multiple of D with len*U/D <= max_len, and gives len*U/D rows: every
 *   call starts on a period boundary (n a multiple of D, the row count a multiple of U).
 *   Taps: 1 <= T <= 16385, |h[j]| <= 32767, and for EVERY phase phi in [0, U) the sum of |h[j]| over j = phi (mod U) is
 *   <= 65535 (else GNUAIS_E_ARG): a row takes the taps of one phase, so the int32 argument above holds per row and any
 *   order of the sums gives the same bits.
 *   Default taps (taps == NULL or n_taps == 0): the formula above with D = down -- T = 16D + 1, the same window,
 *   x[j] = 0.75 * (j - 8D) / D -- scaled by U:  h[j] = rnd(g[j] * 32768.0 * U / G)  (as written, left to right), the same
 *   response at the output rate.  The DC gain of a phase, sum of h[j] over j = phi (mod U), then differs from phase to
 *   phase by rounding: 32758 .. 32828 of 32768 over 24/125, 6/125, 3/64, 2/75, 3/125, 3/128, 12/625, 3/160, 2/125,
 *   3/200, 1/125 and 3/625 (32761 .. 32773 at 24/125).  That is a property of the design, not an error; the largest
 *   per-phase sum |h| is 48604 .. 48776 there (about 50500 at 5/6 and 2/3).
 *   Carried per stream: the last H = ceil((T-1) / U) converted wide samples (T-1 at U = 1); per batch: n.
 * gnuais_batch_resampler(up = 1, down <= 64) IS gnuais_batch_channeliser(down, ...): the same configuration, limits
 * (T <= 1025, sum |h| <= 65535), messages and kernels.  Every wideband entry above and below -- _run_wideband[_fmt][_host],
 * _channelise[_fmt], the node forms, the four sample formats, the AFC, frame times -- works unchanged on a batch
 * configured here; gnuais_batch_channelise writes [len*U/D][N][2]. */
int  gnuais_batch_resampler(gnuais_batch *b, int up, int down, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                            const int16_t *taps, int n_taps);
/* host only, no batch: the default prototype for up / down into out[cap] (*n_taps = 16*down + 1) */
int  gnuais_resampler_default_taps(int up, int down, int16_t *out, int cap, int *n_taps);
/* host only, no batch, for tests: what the device's fast form is planned from (taps NULL / 0 = default).  Rows repeat with
 * period U; row phase i takes the `size` wide samples from `first` on (relative to the period) since the row before:
 * groups[i] = (first, size, base), first = floor((i*D - 1) / U) + 1.  pairs[(base + q) * n_acc + a] = (lo, hi) = the taps
 * of samples k = first + 2q and k + 1 for the row a after this one, j = (i + a)*D + D-1 - k*U, 0 where j is outside
 * [0, T) or the group has no sample k + 1; *n_acc = max(ceil(T / D), 17), the table's stride (17: the accumulators of
 * the device's fast form, whose table this then is), *n_pairs = sum of ceil(size / 2), *carry = H.  Each
 * output may be NULL; groups_cap and pairs_cap count elements (3*up and *n_pairs * *n_acc are needed). */
int  gnuais_resampler_plan(int up, int down, const int16_t *taps, int n_taps, int32_t *groups, int groups_cap,
                           uint32_t *pairs, int pairs_cap, int *n_pairs, int *n_acc, int *carry);

/* ---- sample formats of wideband input: 8-bit and float SDR captures, converted where the channeliser loads them ----
 * Not in the reference.  A sample format says how one wide (I, Q) pair lies in memory and how each of its components
 * becomes the int16 v of the channeliser's definition above:
 *   GNUAIS_FMT_CS16  two little-endian int16 x     v = x: the input of the entries above
 *   GNUAIS_FMT_CU8   two uint8 u (RTL-SDR)         v = 256*u - 32640 = (2u - 255) * 128: zero at 127.5, range +-32640;
 *                                                  on the 16-bit word, (u << 8) ^ 0x8080
 *   GNUAIS_FMT_CS8   two int8 s (HackRF)           v = 256*s, range -32768 .. 32512
 *   GNUAIS_FMT_CF32  two little-endian IEEE fp32 x, full scale +-1.0 (GNU Radio, gqrx, SoapySDR):
 *                                                  y = x * 32768.0f (one fp32 product); r = rint(y), ties to even;
 *                                                  NaN -> 0; v = clamp(r, -32768, 32767), which covers +-inf
 * Everything after the conversion is the channeliser's definition, unchanged, on the converted pairs.  (The 8-bit formats
 * are scaled to full range because the mixer rounds with >> 15: unscaled 8-bit values would vanish in its rounding.)
 * The carry holds converted int16 pairs, so the format is an argument of each call and not a state of the batch: calls of
 * different formats may follow each other on one batch, mixed with cs16, audio and I/Q calls, and the output depends
 * only on the sequence of converted samples -- not on where the stream was cut or on which format carried which part.
 * The input pointer must be aligned to 4 bytes for cs16 and cf32 and to 2 bytes for cu8 and cs8 (else GNUAIS_E_ARG,
 * with a message that names the format); an unknown format is GNUAIS_E_ARG.  len: as above, a positive multiple of D, at
 * most D*max_len.  The entries below are the entries above with the format as an argument (GNUAIS_FMT_CS16 launches
 * exactly what they launch); the _host forms copy the native bytes, len * M * gnuais_sample_format_bytes(fmt). */
#define GNUAIS_FMT_CS16 0
#define GNUAIS_FMT_CU8  1
#define GNUAIS_FMT_CS8  2
#define GNUAIS_FMT_CF32 3
int  gnuais_batch_run_wideband_fmt(gnuais_batch *b, int fmt, const void *d_wide, int len, void *stream);
int  gnuais_batch_run_wideband_fmt_host(gnuais_batch *b, int fmt, const void *h_wide, int len);
int  gnuais_batch_channelise_fmt(gnuais_batch *b, int fmt, const void *d_wide, int len, int16_t *d_out, void *stream);
/* bytes per (I, Q) pair: 4, 2, 2, 8; GNUAIS_E_ARG for an unknown format */
int  gnuais_sample_format_bytes(int fmt);
/* host only, no batch: the table above, in[n_pairs] pairs of `fmt` (any alignment) -> out[n_pairs][2] */
int  gnuais_convert_samples(int fmt, const void *in, size_t n_pairs, int16_t *out);

/* ---- carrier frequency error of I/Q input: an AFC stage on the device between the discriminator and the chain ----
 * Not in the reference (a sound card is AC coupled).  A carrier error of f Hz adds the constant f * 65536 / rate to
 * every discriminator output; an SDR's oscillator is off by several kHz at 162 MHz, more than the AIS deviation, and
 * the slicer decides on the sign alone.  With a window W set, every I/Q-type call (gnuais_batch_run_iq,
 * gnuais_batch_run_wideband, their host forms, gnuais_batch_afc_apply) estimates each channel's error over a centred
 * window and subtracts it; the chain sees the corrected audio delayed by W/2 samples.  Off by default: with W = 0 every
 * call launches the kernels and gives the bits it gives without this section.
 *   W = window in samples, a multiple of 128, 128 <= W <= 16384.  B = 64, Wb = W/64 (even), L = W/2.
 *   Suggested: 2048 at 48 kHz, 8192 at 192 kHz (43 ms; DESIGN.md 4.10 has the decode counts of 512, 1024 and 2048).
 *   n counts the rows that I/Q-type calls have passed to the discriminator since gnuais_batch_afc() or
 *   gnuais_batch_reset().  Per channel, everything integer except the phase of a window sum:
 *     (I, Q) = pair n, (Ip, Qp) = pair n-1, exactly the discriminator's carry ((0, 0) at the start)
 *     r[n] = I*Ip + Q*Qp,  i[n] = Q*Ip - I*Qp           exact integers (r reaches 2^31: wider than int32)
 *     a[n] = the discriminator's output, definition above, unchanged
 *     R_j = sum of r[n], I_j = sum of i[n] over n in [64j, 64j + 64)                          int64 block sums
 *     SR_j = sum of R_k, SI_j = sum of I_k over k in [j - Wb/2, j + Wb/2), R_k = I_k = 0 for k < 0   (|SR| < 2^46)
 *     e_j = the discriminator's formula from ax = |re| onward with re = (float) SR_j, im = (float) SI_j
 *           (int64 -> fp32, round to nearest even); same constants, same order, same rint and clamp; SR = SI = 0 gives 0
 *     output row n: m = n - L;  m < 0: 0;  else out[n] = (int16) (a[m] - e_{m div 64}), two's-complement wrap
 *   (phase arithmetic modulo 2 pi).  Every block that e_{m div 64} needs is complete at row n-1, so a call of len rows
 *   gives len rows and the result does not depend on how the stream is cut into calls.
 * Carried per channel: the last L audio samples, the ring of block sums, the open block; all zero after
 * gnuais_batch_afc() and after gnuais_batch_reset(), which keeps the window.  Audio run calls and
 * gnuais_batch_discriminate() neither read nor change any of it. */
/* window = 0: off (default), else W; other values GNUAIS_E_ARG.  Synchronises the device and clears the AFC state. */
int  gnuais_batch_afc(gnuais_batch *b, int window);
/* e_j of the last output row of each channel (0 before there is one) into h_out[n_channels]; Hz = e * rate / 65536:
 * what to read for an SDR's ppm.  Waits for the last I/Q-type call's AFC stage.  GNUAIS_E_STATE while the AFC is off. */
int  gnuais_batch_afc_estimate(gnuais_batch *b, int16_t *h_out /* [n_channels] */);
/* discriminator + AFC only (a parity tap, as gnuais_batch_discriminate): d_iq DEVICE int16 [len][n_channels][2], d_out
 * DEVICE int16 [len][n_channels]; advances the I/Q carry and the AFC state, nothing else.  Asynchronous on `stream`.
 * GNUAIS_E_STATE while the AFC is off. */
int  gnuais_batch_afc_apply(gnuais_batch *b, const int16_t *d_iq, int len, int16_t *d_out, void *stream);

/* ---- input side, row f2: sample files -> interleaved int16 frames (src/ais.c:173-182,214-217) ---
 * raw_channels > 0: the file is a bare stream of little-endian int16 frames of that many channels,
 *   header and all, exactly as the reference reads a sound file; 0: parse RIFF/WAVE (16-bit PCM,
 *   plain or extensible, any channel count).  gnuais_wav_read(): whole frames read, 0 at the end. */
typedef struct gnuais_wav gnuais_wav;
int  gnuais_wav_open(gnuais_wav **out, const char *path, int raw_channels);
int  gnuais_wav_channels(const gnuais_wav *w);
int  gnuais_wav_rate(const gnuais_wav *w);
long gnuais_wav_read(gnuais_wav *w, int16_t *frames, long max_frames);
void gnuais_wav_close(gnuais_wav *w);

/* ---- stage entry points (parity taps; not needed by a drop-in user) ---------
 * filter_run_buf(), src/filter.c:106-143: d_out = DEVICE float [len][n_channels];
 * advances the FIR history exactly like a run call, nothing else. */
int  gnuais_batch_filter(gnuais_batch *b, const int16_t *d_samples, int len,
			 float *d_out, void *stream);
/* the same from and to HOST memory (plain-C callers: gnuais_amd/csrc/protodec_hip.c): h_samples int16
 * [len][n_channels], h_out float [len][n_channels]; synchronous */
int  gnuais_batch_filter_host(gnuais_batch *b, const int16_t *h_samples, int len, float *h_out);
/* the discriminator only (definition above gnuais_batch_run_iq): d_iq DEVICE int16 [len][n_channels][2], d_out =
 * DEVICE int16 [len][n_channels] (must not overlap d_iq); advances the I/Q carry and nothing else.  Asynchronous on
 * `stream`. */
int  gnuais_batch_discriminate(gnuais_batch *b, const int16_t *d_iq, int len, int16_t *d_out, void *stream);
/* protodec_decode(in, count, d), src/protodec.c:988-1122, for every channel:
 * h_bits = HOST uint8 [n_channels][stride], one byte per bit; h_count[n_channels] */
int  gnuais_batch_decode_bits(gnuais_batch *b, const uint8_t *h_bits, int stride,
			      const int32_t *h_count);
/* recovered (NRZI-decoded) bits of the LAST run call, one byte per bit:
 * h_bits HOST uint8 [n_channels][stride]; h_count[n_channels] = bits per channel */
int  gnuais_batch_last_bits(gnuais_batch *b, uint8_t *h_bits, int stride, int32_t *h_count);

/* the slicer's decisions of the LAST run call (`out > 0`, src/receiver.c:111), one byte per sample:
 * h_out HOST uint8 [n_channels][stride], stride >= len of that call */
int  gnuais_batch_last_signs(gnuais_batch *b, uint8_t *h_out, int stride);
/* facts about a batch, by name: "sign_exact" (1 if the receive path runs the sign-exact slicer),
 * "sign_eps" (its certification threshold), "sign_central_taps", "sign_matrix_pipe" (1 if the batch is ELIGIBLE for
 * the matrix-pipe FIR: table, options and channel count allow it; a call takes it when its length does too),
 * "first_effective_tap",
 * "n_effective_taps", "compute_units", "device", "segments", "pack_bits" (the bits one segment's pack can hold, which
 * follows from pllinc: 64 .. 512; gnuais_batch_decode_bits() feeds "segments" packs of this size per deframer launch),
 * "stream_depth" (calls between a
 * gnuais_batch_stream_nmea() call and the one that hands its text out), "afc_window" (gnuais_batch_afc(); 0 = off),
 * "frame_times" (gnuais_batch_frame_times(); 0 = off), "rows" (rows the chain has taken since create / reset),
 * "frame_signal" (gnuais_batch_frame_signal(); 0 = off), "occupancy" (gnuais_batch_occupancy(); epoch_blocks, 0 = off),
 * "repair" (gnuais_batch_repair(); 0 = off), "long_repair" (gnuais_batch_long_repair(); 0 = off), "long_cand_cap" (the
 * candidate records one call of that repair can list), "unique" (gnuais_batch_unique(); the window, 0 = off), "unique_late"
 * (gnuais_batch_unique_late()), "long_unique" (gnuais_batch_long_unique(); the window, 0 = off), "long_unique_late"
 * (gnuais_batch_long_unique_late()), "pll_form" (the form the PLL launch of the last run call took: 7 the time-parallel
 * one, 8 the lane-per-channel one; 0 before any call and after a reset) */
int  gnuais_batch_info(const gnuais_batch *b, const char *name, double *value);

/* ---- results ------------------------------------------------------------------
 * drain queued frames to the host, in the reference's print order within the
 * drained span (channel 0..N-1, then time).  *n_out = frames written. */
int  gnuais_batch_drain_frames(gnuais_batch *b, gnuais_frame *h_out, int max, int *n_out);
int  gnuais_batch_pending_frames(gnuais_batch *b, int *n_out);
/* stream-ordered: drop everything queued so far without copying it out (the
 * counters keep counting); for consumers that only read counters */
int  gnuais_batch_discard_frames(gnuais_batch *b, void *stream);
int  gnuais_batch_counters(gnuais_batch *b, gnuais_counters *h_out /* [n_channels] */);
int  gnuais_batch_total_received(gnuais_batch *b, long long *total);
/* filter_run_buf()'s return value for the last run: peak positive sample per channel
 * (src/filter.c:118-119; feeds the level log at src/receiver.c:137-147) */
int  gnuais_batch_maxval(gnuais_batch *b, int16_t *h_out /* [n_channels] */);
int  gnuais_batch_pll_state(gnuais_batch *b, gnuais_pll_state *h_out /* [n_channels] */);
int  gnuais_batch_fsm_state(gnuais_batch *b, gnuais_fsm_state *h_out /* [n_channels] */);
/* protodec_reset() (src/protodec.c:87-100) for every decoder of the batch: back to ST_SKURR, the frame in progress
 * dropped, counters untouched.  Synchronises. */
int  gnuais_batch_protodec_reset(gnuais_batch *b);
/* d->buffer of one channel (src/protodec.h:52, written at protodec.c:1019): the stored bits, one per byte, of the frame
 * in progress or -- between frames -- of the last frame that reached its stop bit; *n_bits = their number (may exceed
 * cap: the first cap are written), -1 when neither is on record (no frame yet; the last one given up at 449 bits). */
int  gnuais_batch_frame_bits(gnuais_batch *b, int channel, uint8_t *h_bits, int cap, int *n_bits);
/* the last n_taps input samples per channel, oldest first (live part of
 * struct filter.buffer, src/filter.h:60): h_out int16 [n_channels][n_taps] */
int  gnuais_batch_history(gnuais_batch *b, int16_t *h_out);

/* ---- when a frame was received: its time in input samples ---------------------------------------------------------
 * The reference takes time(&received_t) for every message (src/protodec.c:904-905) and hands it to its cache, its JSON
 * output and its MySQL sink.  A batch delivers a whole call's frames in one drain, and for a recorded capture decoded
 * faster than real time the wall clock says nothing, so the receive time is counted in the input itself.  end_bit
 * counts bits, and the PLL free-runs on noise between bursts: end_bit / 9600 drifts from the capture's clock without
 * bound.  Off by default: while off, a call launches exactly what it launches without this section.
 *   n counts the rows (samples per channel at the chain's rate) the chain has taken since gnuais_batch_create() /
 *   gnuais_batch_reset(), over every kind of run call (audio, I/Q, wideband, their host forms), whether the feature is
 *   on or not.  gnuais_batch_protodec_reset() keeps n as it keeps the bit count.  Row i "slices" when pll > 0xffff
 *   after the add at src/receiver.c:122-124.
 *   A call that takes rows [n0, n0 + len) is cut into segments s = 0, 1, ...: segment s covers the rows
 *   [n0 + 2048 s, n0 + min(2048 (s + 1), len)); l_s is its length, c_s the number of its rows that slice.
 *   The bit with the 37-bit index e = end_bit together with flags[5:1] -- the bit that closed the frame -- is the j-th
 *   slice (counting from 0) of some segment s of the call that fed it.  Its time is
 *     t(e) = n0 + 2048 s + floor((2 j + 1) * l_s / (2 * c_s))                                     int64, exact
 *   independent of which form of the PLL stage ran.  It DOES depend on where the input was cut into calls: a segment
 *   is 2048 rows of a call, not of the stream.
 *   A frame closed by gnuais_batch_decode_bits() (bits without samples), and a frame that was appended while the
 *   feature was off, has t = -1.
 * t is an interpolation inside a segment of 2048 rows, not the slicing row itself: the PLL stage hands on a count per
 * segment and not its phase.  Measured against the true slicing row over every bit of the test inputs
 * the error is within -3 .. +3 rows at 48 kHz (a bit is 5 rows) and -10 .. +10 at 192 kHz (a bit is 20): at most half a
 * bit.  tests/test_frame_times_cpu.py asserts |t - slicing row| <= ceil(65536 / pllinc), one bit period, over those
 * inputs.  That bound is a property of those inputs, not a theorem: the phase nudges of +-pllinc/16 average out on
 * signal and on noise, but an input whose nudges all went one way inside a segment could move the slices of that
 * segment further from an even spread.
 * gnuais_batch_frame_times(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE on a streaming batch, and
 *   while it is on the batch cannot start streaming (gnuais_batch_stream_nmea, gnuais_batch_autotune_delivery and
 *   set_option("streaming", 1) return GNUAIS_E_STATE): streamed sentences carry no times.  One more small launch
 *   follows every call's K3 while it is on.
 * gnuais_batch_drain_frames_timed(): gnuais_batch_drain_frames() with h_times[i] = t of h_out[i].  GNUAIS_E_STATE
 *   while the feature is off.  Every other drain keeps working while it is on (and drops the times with the frames).
 * gnuais_batch_time_map(kind): the input sample index of chain row t is t * mul + off for the batch's configuration at
 *   the time of the call, with d_f = (n_taps + 1) / 2 the centre of the chain FIR's window, W the AFC window (0 = off),
 *   D and T the channeliser's decimation and tap count:
 *     GNUAIS_INPUT_AUDIO      mul = 1,  off = -d_f
 *     GNUAIS_INPUT_IQ         mul = 1,  off = -d_f - W/2
 *     GNUAIS_INPUT_WIDEBAND   mul = D,  off = (-d_f - W/2) * D + D - 1 - (T - 1) / 2     (GNUAIS_E_STATE if not configured,
 *                             and, naming the call below, if gnuais_batch_resampler configured a ratio with up > 1)
 *   The offsets are the delays of the stages as constants -- the nominal decision instant -- not a calibration against
 *   a transmitter's clock.  The index may be negative for the first rows.
 * gnuais_batch_time_map_ratio(kind): the same for every configuration: the input sample index of chain row t is
 *   floor((t * num + off) / den), floor also for negative values.  Audio and I/Q: den = 1, num and off as above.
 *   Wideband: num = D, den = U, off = (-d_f - W/2) * D + D - 1 - (T - 1) div 2 with T the prototype's tap count -- the
 *   map above at U = 1.
 * gnuais_batch_info "frame_times" (0 / 1) and "rows" (n). */
#define GNUAIS_INPUT_AUDIO    0
#define GNUAIS_INPUT_IQ       1
#define GNUAIS_INPUT_WIDEBAND 2
int  gnuais_batch_frame_times(gnuais_batch *b, int on);
int  gnuais_batch_drain_frames_timed(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out);
int  gnuais_batch_time_map(const gnuais_batch *b, int kind, long long *mul, long long *off);
int  gnuais_batch_time_map_ratio(const gnuais_batch *b, int kind, long long *num, long long *den, long long *off);
/* gnuais_nmea_from_frames() with an NMEA 4.10 TAG block in front of EVERY sentence of a frame whose time is known:
 *   \c:<unix>*hh\!AIVDM,...      <unix> = epoch_s + floor((times[i] * mul + off) / rate_hz), decimal, floor also for
 * negative values; hh = XOR of the characters between the backslashes up to the '*', two upper-case hex digits.
 * times[i] = -1: no tag.  mul / off: gnuais_batch_time_map(); rate_hz: the rate of the INPUT samples (> 0); epoch_s:
 * the UNIX second of input sample 0.  With a map from gnuais_batch_time_map_ratio() pass mul = num, off and rate_hz = the
 * input rate * den: floor(floor(a / den) / rate) = floor(a / (den * rate)), so no other entry is needed.  With the tags removed the bytes are those of gnuais_nmea_from_frames(); seqnr,
 * out == NULL and GNUAIS_E_OVERFLOW as there.  Host code. */
int  gnuais_nmea_tagged_from_frames(const gnuais_frame *frames, const int64_t *times, int n_frames, uint8_t *seqnr,
				    int n_channels, long long mul, long long off, long long rate_hz,
				    long long epoch_s, char *out, size_t out_cap, size_t *out_len,
				    int *n_sentences);

/* ---- how strong a frame was and how far off frequency: signal power and carrier error per frame ------------------------
 * Not in the reference (it reads discriminator audio, where a level says nothing).  For I/Q and wideband input every
 * frame gets the mean power of the raw I/Q under it and the power-weighted mean frequency of that I/Q: what an SDR AIS
 * receiver reports per message, what ranks stations, maps coverage and reads an SDR's ppm.  Off by default: while off, a
 * call launches exactly what it launches without this section.  While on, every I/Q-type call launches one more kernel
 * in front of its discriminator, and every call one more behind its frame-time launch.
 * Rows.
 *   n is the chain's row counter (gnuais_batch_info "rows").
 *   x[n] = (I, Q) is the int16 pair an I/Q-type call hands to the discriminator as row n: the caller's pair for
 *   gnuais_batch_run_iq, the channeliser's output pair for gnuais_batch_run_wideband* (and their host forms).
 *   v0 is the first row of the current unbroken run of I/Q-type calls.  It is set to the current n when the feature is
 *   switched on, when gnuais_batch_reset is called, and when the first I/Q-type call follows an audio-type run call.
 *   (While an audio-type run call runs, v0 counts as the row behind that call: its rows are no x[n].)
 *   The previous pair of x[v0] is (0, 0).  This is the stage's own carry, not the discriminator's.
 * Per row, exact integers, (Ip, Qp) = x[n - 1]:
 *   P = I*I + Q*Q (reaches 2^31),  r = I*Ip + Q*Qp,  i = Q*Ip - I*Qp (the AFC's terms; r reaches 2^31)
 * Per block.  Block j covers the rows [64j, 64j + 64) of n.  P_j, R_j and I_j are the int64 sums of P, r and i over the
 *   block.  They are sums of the stream, so they do not depend on where calls are cut.  (Rows of block v0 div 64 that
 *   lie before v0 count as zero; no record below reads that block unless v0 is its first row.)
 * Per frame.  A frame has its time t (gnuais_batch_frame_times) and nbits.  With d_f and W as in
 *   gnuais_batch_time_map(GNUAIS_INPUT_IQ):
 *     q = t - d_f - W/2
 *     S = floor((nbits + 24) * 65536 / pllinc)      payload, CRC and closing flag at the nominal bit length; stuffed
 *                                                   bits only make the burst longer
 *     j_lo = ceil((q - S) / 64),  j_hi = floor((q + 1) / 64),  nb = j_hi - j_lo      (floor and ceil also for negative values)
 *   These are the whole blocks inside [q - S, q].  The record is (0, 0, 0) when t < 0, nb <= 0 or 64 * j_lo < v0.
 *   Otherwise, with the sums over j in [j_lo, j_hi):
 *     power  = floor(sum P_j / (64 * nb)), uint32.  Full scale is 2^31: dBFS = 10 * log10(power / 2^31).
 *     ferr   = the AFC's e formula (above gnuais_batch_afc) on re = (float) sum R_j, im = (float) sum I_j: int64 -> fp32
 *              with round to nearest even, then the discriminator's phase from ax = |re| onward.  int16; Hz = ferr * rate / 65536.
 *     blocks = nb, uint16.
 *   ferr is the power-weighted mean frequency of the raw I/Q over the frame.  The AFC does not change it.  It also carries
 *   the deviation times the imbalance of the frame's own NRZI levels: a property of the estimator (DESIGN.md 4.15 has
 *   the measured spread); no correction for it is made.
 *   Repaired frames get a record like any frame.  Frames of gnuais_batch_decode_bits (t = -1), frames closed by an
 *   audio-type run call and frames appended while the feature was off give (0, 0, 0).
 * gnuais_batch_frame_signal(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE unless frame times are on,
 *   and on a streaming batch; while it is on, gnuais_batch_frame_times(b, 0), the three ways into streaming and
 *   set_option("nbuf") above the depth it was switched on at return GNUAIS_E_STATE.  It allocates a ring of block sums of
 *   24 bytes per channel and block that covers nbuf + 2 calls of max_len rows (GNUAIS_E_HIP with both figures when the
 *   device has no room); switching it off frees the ring.
 * gnuais_batch_drain_frames_signal(): gnuais_batch_drain_frames_timed() with h_signal[i] = the record of h_out[i].
 *   GNUAIS_E_STATE while the feature is off.  Every other drain keeps working while it is on.
 * gnuais_batch_signal_blocks(): a parity tap.  h_out[count][n_channels][3] = (P_j, R_j, I_j) of the blocks
 *   [j0, j0 + count) of the current run.  GNUAIS_E_ARG for blocks the ring does not hold (before block v0 div 64, behind
 *   the last I/Q-type call's rows, or replaced by later ones).  Waits for the last I/Q-type call's ingest.
 * gnuais_frame_signal_span(): the span arithmetic alone, host code: *j_lo and *nb of a frame with time t, or 0 and 0
 *   where the record is (0, 0, 0).  GNUAIS_E_ARG for pllinc = 0 or above 0xffff, nbits outside 0..65535, negative n_taps
 *   or afc_window.
 * gnuais_batch_info "frame_signal" (0 / 1). */
typedef struct gnuais_frame_signal {
	uint32_t power;        /* floor(mean I^2 + Q^2) over the frame's whole blocks; full scale 2^31 */
	int16_t  ferr;         /* carrier error, Hz = ferr * rate / 65536 */
	uint16_t blocks;       /* blocks of 64 rows measured; 0: no measurement, power = ferr = 0 */
} gnuais_frame_signal;
int  gnuais_batch_frame_signal(gnuais_batch *b, int on);
int  gnuais_batch_drain_frames_signal(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, gnuais_frame_signal *h_signal,
                                      int max, int *n_out);
int  gnuais_batch_signal_blocks(gnuais_batch *b, long long j0, int count, int64_t *h_out);
int  gnuais_frame_signal_span(long long t, int nbits, unsigned pllinc, int n_taps, int afc_window, long long v0,
                              long long *j_lo, int *nb);

/* ---- how loaded a channel is: noise floor, busy and decoded air time per receiver -----------------------------------------
 * The section above describes what was decoded.  This one describes what was on the air: per channel and epoch of E
 * blocks, the noise floor, the blocks with a signal above it, how many bursts they form and how many of them lie under a
 * decoded frame -- the load figure of a base station, the reference every `power` is ranked against, and the share of the
 * busy air time that ended in a frame (the rest: collisions, garbled slots, signals too weak to decode).  Off by default:
 * while off, a call launches exactly what it launches without this section.  While on, every I/Q-type call launches one
 * more kernel behind the ingest kernel of the section above and one more behind its frame-signal launch, and the call
 * that makes an epoch final one more per such epoch.
 * n, x[n], P_j, q, S, d_f and W are those of the section above.  v0 is that section's v0, or the row at which
 * gnuais_batch_occupancy switched the feature on where that is later.
 * Code of a block.  code(P) for 0 <= P < 2^38:
 *     code(P) = P                                           for P < 8
 *     code(P) = 8 (e - 2) + ((P >> (e - 3)) & 7)            otherwise, e = floor(log2 P)
 *   monotone, eight steps per octave (0.376 dB), at most 287 (nine bits).
 *     power(code) = code for code < 8, else (8 + (code & 7)) << (code / 8 - 1)         the lower edge of the code's bin
 *   c_j = code(P_j) for every complete block j with 64 j >= v0.
 * Epochs.  b0 = ceil(v0 / 64).  Epoch k of a run covers the blocks [b0 + k E, b0 + (k + 1) E); E is the caller's,
 *   64 <= E <= 4096.
 * Per epoch and channel:
 *     floor   = the element of rank floor(E / 8) (0-based, ascending) among the epoch's c_j.  The lowest octile stays on
 *               noise up to about 85 % load.  Against the mean noise power it is biased low (the octile of a chi-square of
 *               128 degrees, and the bin's lower edge): a property of the estimator (DESIGN.md 4.17 has the measured
 *               value); no correction is made.
 *     busy_j  = c_j >= floor + m, m the caller's margin in code steps, 1 <= m <= 255.
 *     busy    = the number of busy blocks.
 *     bursts  = the number of j in the epoch with busy_j and not busy_(j-1); for the epoch's first block busy_(j-1) is the
 *               value carried from the epoch before (judged with that epoch's floor), 0 for epoch 0 of a run.
 *     cover_j = block j intersects the cover span of a frame with t >= 0 on that channel: the rows
 *               [q - S - S_pre, q + S_post], S_pre = floor(64 * 65536 / pllinc) (ramp, training, start flag, stuffing),
 *               S_post = floor(8 * 65536 / pllinc).  A frame covers only if q - S - S_pre >= v0.  Repaired frames cover
 *               like any frame.
 *     covered = the number of blocks with busy_j and cover_j.
 * When an epoch is final.  At the tail of the first I/Q-type call (rows [n0, n0 + len)) with
 *     n0 + len > 64 (b0 + (k + 1) E) - 1 + LAG,    LAG = floor((448 + 24) * 65536 / pllinc) + S_pre + d_f + W/2 + 64:
 *   every frame that can cover the epoch has its time by then.  The host knows this from n0, len and v0; nothing is read
 *   back to decide it.  A call may make several epochs final, or none.  A run that ends (v0 moves) drops its epochs that
 *   are not final yet; the numbering starts again at the new b0.
 * gnuais_batch_occupancy(epoch_blocks, margin): switches the feature (epoch_blocks = 0: off, the rings are freed);
 *   synchronises the batch.  GNUAIS_E_STATE unless gnuais_batch_frame_signal is on, and on a streaming batch; while it is
 *   on, gnuais_batch_frame_signal(b, 0), set_option("nbuf") above the depth and gnuais_batch_afc() above the window it
 *   was switched on at return GNUAIS_E_STATE.  GNUAIS_E_ARG for values outside the ranges above.  It allocates a ring of
 *   codes and one of cover bytes, 3 bytes per channel and block, of
 *   E + ceil(LAG / 64) + (nbuf + 2) ceil(max_len / 64) + 2 blocks (GNUAIS_E_HIP with the figure when the device has no
 *   room).
 * gnuais_batch_drain_occupancy(): the final epochs not delivered yet, oldest first: h_out[i][c] is the record of channel
 *   c, h_first_block[i] the epoch's first block; *n_out of them, at most max.  Waits for the tails that produced them.
 *   The library holds 64 final epochs; one more overwrites the oldest, which gnuais_batch_occupancy_lost() counts.
 *   gnuais_batch_reset() empties the queue and zeroes that count.
 * gnuais_batch_occupancy_blocks(): a tap, and the occupancy map a caller can plot: h_out[count][n_channels] =
 *   c_j | busy_j << 14 | cover_j << 15 of the blocks [j0, j0 + count).  GNUAIS_E_ARG for blocks that are not of a final
 *   epoch of the current run still held (the codes of later blocks replace them, one ring round later).
 * gnuais_occupancy_code(), gnuais_occupancy_power(), gnuais_occupancy_cover_span(): the arithmetic alone, host code.
 *   code: GNUAIS_E_ARG for P outside 0 .. 2^38 - 1; power: for a code outside 0 .. 288 (288: the upper edge of the last
 *   bin).  cover_span: *j_lo and *nb of the blocks [j_lo, j_lo + nb) the cover span of a frame with time t intersects, or
 *   0 and 0 where it covers nothing; arguments and GNUAIS_E_ARG as for gnuais_frame_signal_span().
 * gnuais_batch_info "occupancy" (epoch_blocks; 0 = off). */
typedef struct gnuais_occupancy {
	uint16_t floor;        /* code of the noise floor; gnuais_occupancy_power(floor) / 64 is a power like gnuais_frame_signal's */
	uint16_t busy;         /* blocks of the epoch at or above floor + margin */
	uint16_t covered;      /* busy blocks under the cover span of a decoded frame */
	uint16_t bursts;       /* runs of busy blocks that begin in the epoch */
} gnuais_occupancy;
int  gnuais_batch_occupancy(gnuais_batch *b, int epoch_blocks, int margin);
int  gnuais_batch_drain_occupancy(gnuais_batch *b, gnuais_occupancy *h_out /* [max][n_channels] */,
                                  int64_t *h_first_block /* [max] */, int max, int *n_out);
int  gnuais_batch_occupancy_lost(gnuais_batch *b, long long *lost);
int  gnuais_batch_occupancy_blocks(gnuais_batch *b, long long j0, int count, uint16_t *h_out /* [count][n_channels] */);
int  gnuais_occupancy_code(long long P, int *code);
int  gnuais_occupancy_power(int code, long long *P);
int  gnuais_occupancy_cover_span(long long t, int nbits, unsigned pllinc, int n_taps, int afc_window, long long v0,
                                 long long *j_lo, int *nb);

/* ---- repair of frames that fail the CRC by one symbol error ---------------------------------------------------------
 * The slicer decides line levels and the NRZI decoder differentiates them, so one wrong level decision is two adjacent
 * wrong bits in the stream the deframer sees.  The reference counts such a frame in lostframes and drops it
 * (src/protodec.c:1105-1108); with the repair on, the frame is looked for among the neighbours of what was received.
 * Off by default: while off, a call launches exactly what it launches without this section.
 *   Candidate.  A record of the deframer's candidate ring that is counted in lostframes: it reached its stop bit with
 *     bufferpos - 22 > 0 and its CRC is wrong.  Its raw bits are r[0 .. rawlen): the bits the deframer saw in ST_DATA,
 *     stuffed zeros included, up to and including the fifth 1 of the closing flag; the sixth 1 is not among them.
 *   Trial p, 0 <= p <= rawlen - 2: r' = r with bits p and p + 1 inverted; ST_DATA of the reference
 *     (src/protodec.c:995-1027, from antallenner = 0, bitstuff = 0, last = 0, bufferpos = 0) runs over r', followed by
 *     one more bit of value 1.
 *   A trial is well formed when that appended bit, and no bit before it, takes the machine to ST_STOPSIGN; bufferpos
 *     never reaches 449; n' = bufferpos - 22 > 0; and n' mod 8 = 0.
 *   A trial passes when it is well formed and protodec_calculate_crc(n') holds on its buffer (the CRC over n'/8 + 2
 *     bytes).
 *   Outcome.  The candidate is repaired iff exactly one trial passes; with none or with several it stays lost.  (Two
 *     trials that leave the stuffing alone cannot both pass: (1 + x)(1 + x^k) is no multiple of the CRC polynomial for
 *     k < 32767.  Several can pass only where a trial makes or destroys a stuffed zero.)  Single-bit flips and two or
 *     more symbol errors are not tried.
 *   The repaired frame is the record the frame would have had, had the deframer stored r': channel; end_bit and
 *     flags[5:1] of the candidate; nbits = n'; payload as for any frame; flags bit 0 and bit 6 (GNUAIS_FRAME_REPAIRED)
 *     set.  It joins the frame ring like any frame (same capacity, same overflow report), takes its place by (channel,
 *     37-bit stamp) in every drain, gets a receive time when gnuais_batch_frame_times is on, and is folded into vessel
 *     tables and sentences like any frame: a consumer that wants received frames only tests bit 6.
 *   Counters.  receivedframes, lostframes and lostframes2 do not move: the frame stays counted in lostframes.  A
 *     per-channel int32 counter `repaired` counts the repairs; gnuais_batch_reset() zeroes it,
 *     gnuais_batch_protodec_reset() keeps it.
 *   False repairs.  A frame with more than one symbol error is accepted wrongly with probability about trials / 65536
 *     (under one per cent); no message-type plausibility check is made.
 * gnuais_batch_repair(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE on a streaming batch, and
 *   while it is on the batch cannot start streaming (gnuais_batch_stream_nmea, gnuais_batch_autotune_delivery and
 *   set_option("streaming", 1) return GNUAIS_E_STATE): the streamed delivery's order table describes the CRC stage's
 *   records only.  One more launch follows every call's CRC stage while it is on (and every chunk of
 *   gnuais_batch_decode_bits).
 * gnuais_batch_repaired(): h_out[c] = repairs on channel c since create / reset.  Synchronises.
 * gnuais_repair_candidate(): the same repair of one candidate on the host, from its raw bits (one per byte, bit 0
 *   counts; n_raw <= 576).  Returns the number of passing trials, or GNUAIS_E_ARG; when that number is 1, payload[53]
 *   (zero behind nbits / 8 bytes), *nbits = n' and *pos = p are written.  It does not ask whether r itself passes.
 *   Host code, no device. */
int  gnuais_batch_repair(gnuais_batch *b, int on);
int  gnuais_batch_repaired(gnuais_batch *b, int32_t *h_out /* [n_channels] */);
int  gnuais_repair_candidate(const uint8_t *raw_bits, int n_raw, uint8_t payload[53], int *nbits, int *pos);

/* ---- messages of three to five slots: a second decoder for long frames ------------------------------------------------
 * protodec_decode() gives a frame up once 449 unstuffed bits are stored (src/protodec.c:1024), so the chain -- which is the
 * reference bit for bit -- delivers no message of more than 426 bits: two slots.  ITU-R M.1371 allows five slots, 1008
 * bits: binary messages (types 6, 8), safety text (12, 14), DGNSS corrections (17), type 26.  With this feature on they are
 * delivered as records of their own.  Off by default: while off, a call launches exactly what it launches without this
 * section, and whether on or off the chain's frames, counters and state are what they are without it.
 *   Definition.  Each channel gets a second decoder D', independent of the chain's.  It is protodec_decode() /
 *     protodec_reset() / protodec_calculate_crc() statement by statement with exactly these changes:
 *       - the two buffers hold 1200 bits;
 *       - the give-up test `bufferpos >= 449` is `bufferpos >= 1031`: GNUAIS_LONG_MAX_BITS + 22 + 1;
 *       - a frame that reaches ST_STOPSIGN's good branch (stop bit 0, n = bufferpos - 22 > 0) is delivered only if
 *         n > 426 and the CRC holds -- the reference's routine over n/8 + 2 bytes, as it stands.  Frames with n <= 426
 *         belong to the chain's decoder: D' walks over them and says nothing;
 *       - D' keeps two per-channel int32 counters: long frames delivered, and long frames (n > 426) that failed the CRC.
 *   Carried state.  D' sees the bit stream the chain's deframer sees, through every kind of call: audio, I/Q, wideband,
 *     their host forms, gnuais_batch_decode_bits.  Its bit count IS that deframer's count: a long frame's 37-bit stamp
 *     (end_bit and flags[5:1]) is what the chain's deframer would stamp a frame closing on the same bit, also when the
 *     feature is switched on in mid-stream, and gnuais_batch_set_clock moves it.  gnuais_batch_reset() clears everything;
 *     gnuais_batch_protodec_reset() resets D''s machine and keeps the count and the counters.  Switching the feature on or
 *     off synchronises and resets D''s machine, ring and counters.
 *   Record.  payload is packed as in gnuais_frame: nbits/8 bytes used, the rest zero.  flags bit 0 is set, bits 5:1 are
 *     stamp bits 36:32.  t is the receive time by the formula of the frame-times section, n_0 + 2048 s + floor((2j + 1)
 *     l_s / (2 c_s)): D''s kernel walks a call's segments in order and knows s, j, l_s and c_s of the closing bit itself,
 *     so t is filled in whether gnuais_batch_frame_times is on or off.  t = -1 for a frame closed by
 *     gnuais_batch_decode_bits.
 *   Not in this section.  The duplicate merge and the member lists of the long frames have a section of their own
 *     (gnuais_batch_long_unique, below), and so have their signal records and their share in the channel load
 *     (gnuais_batch_long_frame_signal, below).  For long frames there is no stdout text line, no device formatter
 *     (gnuais_batch_drain_nmea and its family), no entry in the vessel tables and no streamed delivery.  t and the stamp
 *     are in the record, so a host can do these itself.
 * gnuais_batch_long_frames(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE on a streaming batch, and
 *   while it is on the batch cannot start streaming (gnuais_batch_stream_nmea, gnuais_batch_autotune_delivery and
 *   set_option("streaming", 1) return GNUAIS_E_STATE): the streamed delivery carries no records of long frames.  One more
 *   launch follows every call's CRC stage while it is on (and every chunk of gnuais_batch_decode_bits).
 * gnuais_batch_pending_long_frames(): the long frames queued.  Synchronises.
 * gnuais_batch_drain_long_frames(): everything queued, consumed once, in (channel, stamp) order.  The long frames have a
 *   ring of their own (info "long_frame_cap": sized from max_len and pllinc so that the worst case of one call fits -- a
 *   long burst is at least about 470 bits); when it overflowed the call delivers what it holds, the oldest records, and
 *   returns GNUAIS_E_OVERFLOW, as the frame ring does.  GNUAIS_E_ARG when max is less than what is queued.
 * gnuais_batch_long_counters(): the two counters of D' per channel since create / reset / the last switch.
 * gnuais_batch_long_fsm_state(): the live fields of D''s machine, as gnuais_batch_fsm_state() (bufferpos up to 1030):
 *   the parity tap for the carried state.
 *   These four return GNUAIS_E_STATE on a batch whose feature was never switched on.
 * gnuais_nmea_from_long_frames(): host code, no device.  protodec_getdata()'s head (type test, fill bits, sequence digit)
 *   and protodec_generate_nmea() as written (src/protodec.c:780-926) over the longer buffer: two or three sentences of at
 *   most 61 characters per frame.  seqnr, sizing and overflow as in gnuais_nmea_from_frames(); a caller may pass the
 *   same seqnr array to both.  GNUAIS_E_ARG for a record with nbits > GNUAIS_LONG_MAX_BITS. */
#define GNUAIS_LONG_MAX_BITS 1008
typedef struct gnuais_long_frame {
	uint32_t channel, end_bit;
	int64_t  t;
	uint16_t nbits;
	uint8_t  flags, reserved;
	uint8_t  payload[132];
} gnuais_long_frame;   /* 152 bytes */
int  gnuais_batch_long_frames(gnuais_batch *b, int on);
int  gnuais_batch_pending_long_frames(gnuais_batch *b, int *n_out);
int  gnuais_batch_drain_long_frames(gnuais_batch *b, gnuais_long_frame *h_out, int max, int *n_out);
int  gnuais_batch_long_counters(gnuais_batch *b, int32_t *h_delivered /* [n_channels] */, int32_t *h_failed /* [n_channels] */);
int  gnuais_batch_long_fsm_state(gnuais_batch *b, gnuais_fsm_state *h_out /* [n_channels] */);
int  gnuais_nmea_from_long_frames(const gnuais_long_frame *frames, int n_frames, uint8_t *seqnr, int n_channels,
                                  char *out, size_t out_cap, size_t *out_len, int *n_sentences);

/* ---- repair of long frames that fail the CRC by one symbol error -------------------------------------------------------
 * A 1008-bit frame carries about five times the symbols of a position report, so at the same symbol error rate it fails
 * its CRC about five times as often; D' counts such a frame in `failed` and drops it.  With this repair on, the frame is
 * looked for among the pair-flip neighbours of what was received, as gnuais_batch_repair does for the chain's frames (one
 * wrong level decision is two adjacent wrong bits behind the NRZI decoder).  The section mirrors that one statement by
 * statement, with D''s numbers.  Off by default: while off, a call launches exactly what it launches without this
 * section, and no result of the sections above changes.  gnuais_batch_repair keeps its meaning: the chain's frames only.
 *   Candidate.  A frame that D' counts in `failed`: it reached ST_STOPSIGN's good branch (stop bit 0) with
 *     n = bufferpos - 22 > 426 and its CRC is wrong; n need not be a multiple of 8.  Its raw bits are r[0 .. rawlen): the
 *     bits D' saw in ST_DATA, stuffed zeros included, up to and including the fifth 1 of the closing flag; the sixth 1 is
 *     not among them.  rawlen <= 1236: 1030 stored bits and at most 206 stuffed zeros, 40 words.
 *   Trial p, 0 <= p <= rawlen - 2: r' = r with bits p and p + 1 inverted; ST_DATA of D' (from antallenner = 0,
 *     bitstuff = 0, last = 0, bufferpos = 0) runs over r', followed by one more bit of value 1.
 *   A trial is well formed when that appended bit, and no bit before it, takes the machine to ST_STOPSIGN; bufferpos
 *     never reaches 1031; and n' = bufferpos - 22 satisfies 426 < n' <= 1008 and n' mod 8 = 0.
 *   A trial passes when it is well formed and the reference's CRC over n'/8 + 2 bytes of its buffer holds.
 *   Outcome.  The candidate is repaired iff exactly one trial passes; with none or with several it stays lost.
 *     Single-bit flips and two or more symbol errors are not tried.
 *   Record.  The repaired frame is a gnuais_long_frame in the long ring: the candidate's channel, stamp (end_bit and
 *     flags[5:1]) and t; nbits = n'; the payload of r'; flags bit 0 and bit 6 (GNUAIS_FRAME_REPAIRED) set.  It shares the
 *     ring's capacity and overflow report, drains in (channel, stamp) order with the others, and
 *     gnuais_nmea_from_long_frames takes it as it takes any record: a consumer that wants received frames only tests bit 6.
 *   Counters.  D''s two counters do not move: the frame stays counted in `failed`.  A third per-channel int32 counter,
 *     long_repaired, counts the repairs, with the reset rules of the other two: gnuais_batch_reset() and a switch of
 *     gnuais_batch_long_frames zero it, gnuais_batch_protodec_reset() keeps it.  Switching the repair itself leaves it.
 *   False repairs.  A frame with more than one symbol error is accepted wrongly with probability about trials / 65536,
 *     at most 1235 / 65536, about 1.9 per cent for the longest frame; no message-type plausibility check is made.
 *   Against the chain's repair.  n' > 426 keeps the two disjoint.  A 424-bit frame whose error destroyed stuffed zeros can
 *     be a candidate here with n = 427 or more; its only passing trial gives n' = 424, which is not delivered here: the
 *     chain's repair owns it.  A 432-bit frame whose error made a stuffed zero has n = 431; the chain gave it up at 449
 *     stored bits, and it is repaired here.
 * gnuais_batch_long_repair(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE unless
 *   gnuais_batch_long_frames is on, and on a streaming batch; switching long frames off switches it off.  While it is on
 *   D' runs in a form that keeps the raw bits of a closing frame and lists the failed ones, and one more launch follows
 *   D''s (also behind every chunk of gnuais_batch_decode_bits).  info "long_repair" and "long_cand_cap": the switch, and
 *   the records the candidate list of one call holds (sized like the long ring; consumed within the call).
 * gnuais_batch_long_repaired(): h_out[c] = long frames repaired on channel c.  Synchronises.  GNUAIS_E_STATE on a batch
 *   that never decoded long frames.
 * gnuais_long_repair_candidate(): the same repair of one candidate on the host, from its raw bits (one per byte, bit 0
 *   counts; n_raw <= 1280, more gives 0).  Returns the number of passing trials, or GNUAIS_E_ARG; when that number is 1,
 *   payload[126] (zero behind nbits / 8 bytes), *nbits = n' and *pos = p are written.  It does not ask whether r itself
 *   passes.  Host code, no device. */
int  gnuais_batch_long_repair(gnuais_batch *b, int on);
int  gnuais_batch_long_repaired(gnuais_batch *b, int32_t *h_out /* [n_channels] */);
int  gnuais_long_repair_candidate(const uint8_t *raw_bits, int n_raw, uint8_t payload[126], int *nbits, int *pos);

/* ---- each transmission once: the copies several receivers hear, merged on the delivery side ----------------------------
 * Not in the reference (one process, one or two receivers).  A batch is thousands of receivers with overlapping cover,
 * and most transmissions are heard by more than one of them; every copy is a frame of its own in the drains above.
 * With a window W set, gnuais_batch_drain_frames_unique() delivers one record per cluster of equal frames, with the
 * number of copies.  Off by default; nothing runs per call, the stage is the drain; every other entry is unchanged.
 *   Key of a frame: nbits and the 53 payload bytes.  channel, end_bit and flags are not part of it: a repaired and an
 *     intact copy share a key.
 *   Member order: within one key, the frames with t >= 0 (gnuais_batch_frame_times) ordered by (t, channel).  The order
 *     is total: two frames of one channel never share a t, the slices of a segment map to strictly increasing rows.
 *   Chain rule: with W > 0 rows, member i belongs to the cluster of member i - 1 iff t_i - t_{i-1} <= W.  A cluster is
 *     a maximal run: a chain may span more than W from its first to its last member.
 *   Primary: the first member of the cluster in the order (flags bit 6, t, channel) -- the earliest intact copy, or the
 *     earliest repaired one when all are repaired.  The delivered record and time are the primary's own, unchanged;
 *     copies = the cluster's size.
 *   Untimed frames: a frame with t = -1 (gnuais_batch_decode_bits, or appended while times were off) is a cluster by
 *     itself, copies = 1.
 *   Output order: the t = -1 frames first, in the plain drain's order (channel, then the 37-bit stamp); the rest by
 *     (t, channel) of the primary.
 *   Across drains: let n = "rows" at the drain.  THE PROPERTY RELIED ON: every time of a drain lies in [rows before the
 *     first call it covers, n), so every frame of a later drain has t >= n (a frame's time is a row of the call that
 *     closed it; tests/test_unique_cpu.py asserts it on the times' reference).  A cluster whose last member has
 *     t_last + W >= n stays open as a tail entry (key, t_last).  In the next drain a tail entry is a virtual first
 *     member of its key: frames that chain onto it are late copies of a transmission already delivered -- they are not
 *     delivered, they are counted in a 64-bit counter `late`, and they move t_last forward.  Tail entries with
 *     t_last + W < n are dropped at the end of a drain.  So for any placement of the drains, sum(copies) + late = the
 *     frames gnuais_batch_drain_frames_timed() would have delivered, and the set of clusters is that of one drain over
 *     everything; only copies against late, and which member is the primary, depend on the cuts.
 *   State: gnuais_batch_reset() and switching the feature (off, on, or to another window) clear the tail and `late`;
 *     gnuais_batch_protodec_reset() keeps both.  Frames consumed by any other drain, or dropped by
 *     gnuais_batch_discard_frames(), are never seen by the stage.
 *   Clocks: all channels of a batch share the row clock; aligning receivers whose captures start at different
 *     instants is the caller's business.
 *   Exactness: the device groups by a 64-bit hash of the key and then compares the keys themselves; where two
 *     different keys share a hash the drain repeats its grouping by the key words, so the result is the definition's
 *     for every input (set_option("unique_hash_bits", k) truncates the hash to k bits to exercise that path).  No
 *     result depends on the order in which the frames entered the ring.
 * gnuais_batch_unique(window_rows): > 0 switches the feature on with that window, 0 off; synchronises.  GNUAIS_E_STATE
 *   unless frame times are on, and on a streaming batch.  While it is on, gnuais_batch_frame_times(b, 0) and the three
 *   ways into streaming return GNUAIS_E_STATE.
 * gnuais_batch_drain_frames_unique(): consumes the queued frames like gnuais_batch_drain_frames(); h_out[i], h_times[i],
 *   h_copies[i] describe cluster i.  GNUAIS_E_STATE while the feature is off; GNUAIS_E_ARG, consuming nothing, when max
 *   is smaller than the number of pending frames (the upper bound); overflow and watchdog are reported late, as there.
 *   76 bytes per delivered record cross PCIe.
 * gnuais_batch_unique_late(): `late` since the feature was switched on / the last reset.
 * gnuais_uniq: the same merge as a host object, no device: _push() is one drain of the definition over frames[n] /
 *   times[n] in any order with rows = n of the definition; at most cap records are written (GNUAIS_E_ARG, with the
 *   object unchanged, when the push would deliver more).  The device drain equals it bit for bit. */
int  gnuais_batch_unique(gnuais_batch *b, int window_rows);
int  gnuais_batch_drain_frames_unique(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                      int *n_out);
int  gnuais_batch_unique_late(gnuais_batch *b, long long *late);
typedef struct gnuais_uniq gnuais_uniq;
int  gnuais_uniq_create(gnuais_uniq **out, long long window);
void gnuais_uniq_destroy(gnuais_uniq *u);
int  gnuais_uniq_reset(gnuais_uniq *u);
int  gnuais_uniq_push(gnuais_uniq *u, const gnuais_frame *frames, const int64_t *times, int n, long long rows,
                      gnuais_frame *out, int64_t *out_times, int32_t *out_copies, int cap, int *n_out);
long long gnuais_uniq_late(const gnuais_uniq *u);

/* ---- who heard each transmission: the unique drain with its clusters' member lists ----------------------------------
 * gnuais_batch_drain_frames_heard() is gnuais_batch_drain_frames_unique() with, for every delivered cluster, the list
 * of its members in CSR form.  Same feature switch (gnuais_batch_unique), same states, same errors, same max rule.
 *   h_out, h_times, h_copies, *n_out: those of gnuais_batch_drain_frames_unique() for the same state, byte for byte.
 *   h_first[max + 1]: h_first[0] = 0 and h_first[i + 1] - h_first[i] = h_copies[i].
 *   h_members[max]: cluster i's members are h_members[h_first[i] .. h_first[i + 1]), in the member order (t, channel)
 *     of the definition above.  sum(copies) <= pending <= max, so max members always suffice.
 *   *n_members = h_first[*n_out].
 *   A member is the copy's receiver (channel), the copy's own gnuais_frame.flags (bit 6: this copy was repaired), its
 *     receive time and its signal record -- (0, 0, 0) while gnuais_batch_frame_signal is off, and wherever that
 *     section gives (0, 0, 0).
 *   An untimed frame is a cluster of one member with t = -1.
 *   The primary is one of the members: the one whose channel and t are those of h_out[i] and h_times[i].  The primary
 *     rule does not change; a caller that wants the strongest copy picks it from the list.
 *   Late copies chain onto a tail entry of an earlier drain; they stay what they are: counted in `late`, listed
 *     nowhere.  A cluster is listed by the drain that delivers it, with the members that drain saw.
 *   State: the carried state (tail, `late`) is the one state of the feature; the two drains may be mixed freely from
 *     drain to drain.  Over any placement of drains of either kind, the listed members plus `late` are the frames
 *     gnuais_batch_drain_frames_timed() would have delivered.
 *   No result depends on the order in which frames entered the ring, nor on the hash.
 *   76 + 4 bytes per delivered record and 24 per member cross PCIe.
 * gnuais_uniq_push_heard(): gnuais_uniq_push() with the lists; its first three outputs and *n_out equal _push()'s.
 *   signal[n] are the frames' records, NULL for zeros.  out_first has cap + 1 entries, out_members n (one per pushed
 *   frame always suffices).  On GNUAIS_E_ARG the object is unchanged.  The device drain equals it bit for bit. */
typedef struct gnuais_hearer {      /* 24 bytes */
	uint32_t channel;               /* the copy's receiver */
	uint32_t flags;                 /* the copy's gnuais_frame.flags (bit 6: this copy was repaired) */
	int64_t  t;                     /* the copy's receive time, -1 for an untimed frame */
	gnuais_frame_signal signal;     /* the copy's record; (0,0,0) while gnuais_batch_frame_signal is off */
} gnuais_hearer;
int  gnuais_batch_drain_frames_heard(gnuais_batch *b, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies,
                                     int max, int *n_out,
                                     int32_t *h_first /* [max + 1] */, gnuais_hearer *h_members /* [max] */,
                                     int *n_members);
int  gnuais_uniq_push_heard(gnuais_uniq *u, const gnuais_frame *frames, const int64_t *times,
                            const gnuais_frame_signal *signal /* NULL: zeros */, int n, long long rows, gnuais_frame *out,
                            int64_t *out_times, int32_t *out_copies, int cap, int *n_out, int32_t *out_first,
                            gnuais_hearer *out_members, int *n_members);

/* ---- each long transmission once: the copies of the long frames merged, with who heard them -----------------------------
 * Long messages are broadcasts -- area notices and met/hydro data (type 8), DGNSS corrections (17), safety text (14) -- and
 * a whole region of receivers hears each one.  This section is gnuais_batch_unique and gnuais_batch_drain_frames_heard
 * for the records of gnuais_batch_long_frames, statement by statement, with exactly these differences.  Off by default;
 * nothing runs per call, the stage is the drain; every other entry is unchanged.
 *   Record words.  A gnuais_long_frame is 38 32-bit words: w0 channel, w1 end_bit, w2..3 t, w4 nbits | flags << 16 |
 *     reserved << 24, w5..37 the 132 payload bytes.
 *   Key of a long frame: nbits and the 132 payload bytes: w4 & 0xffff and w5..w37 -- 34 words, 17 pairs.  channel,
 *     end_bit, t, flags and reserved are not part of it: an intact copy and a repaired copy (GNUAIS_FRAME_REPAIRED, flags
 *     bit 6, from gnuais_batch_long_repair) share a key.
 *   Time.  The member time is the record's own t, which D' always fills: gnuais_batch_frame_times is NOT needed.  A
 *     record with t = -1 (a frame closed by gnuais_batch_decode_bits) is a cluster by itself, copies = 1; those clusters
 *     come first in the output, in the plain long drain's order (channel, then the 37-bit stamp).
 *   Taken over unchanged: the member order (t, channel); the chain rule t_i - t_{i-1} <= W; the primary, the first member
 *     in (flags bit 6, t, channel); the output order of the timed primaries, (t, channel); the tail rule across drains
 *     with n = "rows" of the batch; `late`, the copies that chain onto a tail entry; a cluster is listed by the drain that
 *     delivers it; no result depends on the hash or on the order in which records entered the ring.
 *   THE PROPERTY RELIED ON across drains: every t of a drain lies in [rows before the first call it covers, rows at the
 *     drain): D' computes t by the frame-time formula at its closing bit, a row of the call that closed the frame
 *     (tests/test_long_unique_cpu.py asserts it on the reference).
 *   Member: a gnuais_hearer -- channel, the copy's own flags, the copy's t, and the copy's signal record: that of
 *     gnuais_batch_long_frame_signal (below) while it is on, (0, 0, 0) while it is off.
 *   State.  The long stage has a tail and a `late` counter of its own, independent of gnuais_batch_unique's.
 *     gnuais_batch_reset() clears both; gnuais_batch_protodec_reset() keeps both; any switch of gnuais_batch_long_frames
 *     clears them, and switching long frames off switches this feature off, as it does gnuais_batch_long_repair;
 *     switching the feature itself (off, on, or to another window) clears them.  Records consumed by
 *     gnuais_batch_drain_long_frames() are never seen by the stage; that drain and the two below may be mixed from drain
 *     to drain.
 *   Invariant.  Over any placement of drains, sum(copies) + late = the records gnuais_batch_drain_long_frames() would
 *     have delivered, and the set of clusters is that of one drain over everything.
 *   Exactness: as above; where two different keys share a hash the drain repeats its grouping by the 17 pairs of key
 *     words.  set_option("unique_hash_bits", k) truncates this stage's hash too.
 * gnuais_batch_long_unique(window_rows): > 0 switches the feature on with that window, 0 off; synchronises.
 *   GNUAIS_E_STATE unless gnuais_batch_long_frames is on.  info "long_unique" (the window, 0 = off) and "long_unique_late".
 * gnuais_batch_drain_long_frames_unique(): consumes the queued long frames like gnuais_batch_drain_long_frames();
 *   h_out[i], h_copies[i] describe cluster i.  GNUAIS_E_STATE while the feature is off; GNUAIS_E_ARG, consuming nothing
 *   and leaving tail and `late` unchanged, when max is smaller than the number of pending long frames (the upper bound).
 *   A ring that overflowed is reported as gnuais_batch_drain_long_frames() reports it: GNUAIS_E_OVERFLOW, with what the
 *   ring held, merged.  156 bytes per delivered record cross PCIe.
 * gnuais_batch_drain_long_frames_heard(): the same drain with the clusters' member lists in CSR form, as
 *   gnuais_batch_drain_frames_heard(): h_first[0] = 0, h_first[i + 1] - h_first[i] = h_copies[i], cluster i's members are
 *   h_members[h_first[i] .. h_first[i + 1]) in member order, *n_members = h_first[*n_out]; its first two outputs and
 *   *n_out are those of the unique drain for the same state, byte for byte.  4 more bytes per record and 24 per member
 *   cross PCIe.
 * gnuais_batch_long_unique_late(): `late` since the feature was switched on / the last reset.
 * gnuais_long_uniq: the same merge as a host object, no device: _push() is one drain of the definition over frames[n] in
 *   any order with rows = n of the definition; at most cap records are written (GNUAIS_E_ARG, with the object unchanged,
 *   when the push would deliver more).  _push_heard(): with the lists; out_first has cap + 1 entries, out_members n.
 *   _push_heard_signal(): _push_heard() with signal[n], the frames' records (gnuais_batch_long_frame_signal), in the
 *   members; NULL gives zeros, and then it equals _push_heard() byte for byte.  The device drains equal them bit for bit. */
int  gnuais_batch_long_unique(gnuais_batch *b, int window_rows);
int  gnuais_batch_drain_long_frames_unique(gnuais_batch *b, gnuais_long_frame *h_out, int32_t *h_copies, int max,
                                           int *n_out);
int  gnuais_batch_drain_long_frames_heard(gnuais_batch *b, gnuais_long_frame *h_out, int32_t *h_copies, int max,
                                          int *n_out, int32_t *h_first /* [max + 1] */,
                                          gnuais_hearer *h_members /* [max] */, int *n_members);
int  gnuais_batch_long_unique_late(gnuais_batch *b, long long *late);
typedef struct gnuais_long_uniq gnuais_long_uniq;
int  gnuais_long_uniq_create(gnuais_long_uniq **out, long long window);
void gnuais_long_uniq_destroy(gnuais_long_uniq *u);
int  gnuais_long_uniq_reset(gnuais_long_uniq *u);
int  gnuais_long_uniq_push(gnuais_long_uniq *u, const gnuais_long_frame *frames, int n, long long rows,
                           gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out);
int  gnuais_long_uniq_push_heard(gnuais_long_uniq *u, const gnuais_long_frame *frames, int n, long long rows,
                                 gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out, int32_t *out_first,
                                 gnuais_hearer *out_members, int *n_members);
int  gnuais_long_uniq_push_heard_signal(gnuais_long_uniq *u, const gnuais_long_frame *frames,
                                        const gnuais_frame_signal *signal /* NULL: zeros */, int n, long long rows,
                                        gnuais_long_frame *out, int32_t *out_copies, int cap, int *n_out, int32_t *out_first,
                                        gnuais_hearer *out_members, int *n_members);
long long gnuais_long_uniq_late(const gnuais_long_uniq *u);

/* ---- how strong a long frame was: signal power, carrier error and channel-load share for long frames ---------------------
 * The records of gnuais_batch_long_frames get what gnuais_batch_frame_signal gives the chain's frames, from the same ring
 * of block sums, and cover their air time in gnuais_batch_occupancy.  Off by default: while off, a call launches exactly
 * what it launches without this section and every result above is what it is without it.  While on, every call launches
 * one more kernel behind D' and, where gnuais_batch_long_repair is on, behind the repair launch.
 *   Record.  A long record with time t and nbits gets a gnuais_frame_signal by exactly the formulas of the
 *     gnuais_batch_frame_signal section: q, S = floor((nbits + 24) * 65536 / pllinc), j_lo, j_hi, nb, power, ferr, blocks,
 *     with the same n, x[n], block sums and v0.  Repaired records count, with their own n' and the candidate's t.  nb is
 *     up to 81 at 48 kHz.  gnuais_frame_signal_span() is the span arithmetic for any nbits up to 65535: it has no long twin.
 *     The record is (0, 0, 0) when t < 0 (frames of gnuais_batch_decode_bits), nb <= 0 or 64 * j_lo < v0; for frames closed
 *     by an audio-type run call; and for records appended while the feature was off.
 *   Channel load.  When gnuais_batch_occupancy is switched on while this feature is on, cover_j also counts the long
 *     records -- the same cover span [q - S - S_pre, q + S_post] with the record's own nbits, covering only if
 *     q - S - S_pre >= v0 -- and LAG takes GNUAIS_LONG_MAX_BITS + 24 in place of 448 + 24:
 *       LAG = floor((1008 + 24) * 65536 / pllinc) + S_pre + d_f + W/2 + 64;
 *     the ring sizes follow that LAG (info "occupancy_lag": LAG in rows, of the rings in use, else of the next switch).
 *     The call's epoch finalisers then run behind the long frames' cover: chain cover, D', long repair, long signal and
 *     cover, finalisers.  With this feature off when occupancy is switched on, LAG, sizes and results are what they are
 *     without this section.
 * gnuais_batch_long_frame_signal(on): switches the feature; synchronises the batch.  GNUAIS_E_STATE unless
 *   gnuais_batch_long_frames and gnuais_batch_frame_signal are on, and -- in either direction -- while
 *   gnuais_batch_occupancy is on (its rings are sized by LAG).  While it is on gnuais_batch_frame_signal(b, 0) returns
 *   GNUAIS_E_STATE; gnuais_batch_long_frames(b, 0) switches it off, as it does gnuais_batch_long_repair.  Switching on
 *   re-sizes the ring of block sums for the span of GNUAIS_LONG_MAX_BITS bits in place of 448 and starts a new run (v0 =
 *   the current row), exactly as switching gnuais_batch_frame_signal on does; the records of frames already queued stay
 *   as they are (long ones: (0, 0, 0)).  Switching off keeps the larger ring until gnuais_batch_frame_signal is switched.
 * gnuais_batch_drain_long_frames_signal(): gnuais_batch_drain_long_frames() with h_signal[i] = the record of h_out[i].
 *   GNUAIS_E_STATE while the feature is off.  Every other drain keeps working while it is on;
 *   gnuais_batch_drain_long_frames_heard() then carries each copy's record in its members.
 * gnuais_batch_info "long_frame_signal" (0 / 1) and "occupancy_lag". */
int  gnuais_batch_long_frame_signal(gnuais_batch *b, int on);
int  gnuais_batch_drain_long_frames_signal(gnuais_batch *b, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max,
                                           int *n_out);

int  gnuais_batch_n_channels(const gnuais_batch *b);
int  gnuais_batch_n_taps(const gnuais_batch *b);

/* ---- misc -------------------------------------------------------------------- */
/* the reference coefficient table, src/receiver.c:39-50, rounded to fp32 */
int  gnuais_default_taps(float *out36);
/* CRC-16/X-25 on the device (protodec_sdlc_crc, src/protodec.c:106-118):
 * h_data = n_msgs rows of `stride` bytes, h_len[n_msgs]; h_crc[n_msgs] */
int  gnuais_crc16_batch(int device, const uint8_t *h_data, int stride, const int32_t *h_len,
			int n_msgs, uint16_t *h_crc);
/* protodec_calculate_crc's arithmetic (src/protodec.c:120-167) for one frame in one device call:
 * h_bits = 8 * n_bytes cells of one bit each, as the deframer leaves them in d->buffer (the first
 * cell of a byte is its least significant bit, src/protodec.c:138-143); *h_crc = CRC-16/X-25 over the
 * n_bytes bytes (a good frame + FCS gives 0x0f47, src/protodec.c:166); h_msb receives the first n_out
 * cells byte by byte with the most significant bit first (d->rbuffer, src/protodec.c:150-162;
 * n_out = 0: not wanted).  1 <= n_bytes <= 64, n_out <= 8 * n_bytes. */
int  gnuais_crc16_bits(int device, const uint8_t *h_bits, int n_bytes, uint16_t *h_crc,
		       uint8_t *h_msb, int n_out);
/* Row f1, first part -- the NMEA 0183 sentences of CRC-valid frames, byte-identical to what the
 * reference passes to serial_write() (protodec_getdata src/protodec.c:896-926 +
 * protodec_generate_nmea src/protodec.c:780-894).  Host-side, like the reference's own
 * post-stage.  frames[n_frames] in delivery order (gnuais_batch_drain_frames);
 * seqnr[n_channels] is the per-receiver rolling sequence digit d->seqnr (in/out, start at 0).
 * Sentences are written back to back, each "!AIVDM,...*hh\r\n".  *out_len = bytes needed;
 * out == NULL only sizes (seqnr still advances); too small a buffer -> GNUAIS_E_OVERFLOW. */
int  gnuais_nmea_from_frames(const gnuais_frame *frames, int n_frames, uint8_t *seqnr,
			     int n_channels, char *out, size_t out_cap, size_t *out_len,
			     int *n_sentences);
/* Row f1, complete -- everything protodec_getdata() (src/protodec.c:896-986) produces for CRC-valid
 * frames: the NMEA sentences as above, and the line it prints on stdout for each accepted frame:
 * "ch <id> type <t> mmsi <9 digits>:" + the fields of the per-type decoders (src/protodec.c:357-776)
 * + " (!<last sentence>)\n".  chanid[n_channels] are the receivers' names (receiver.h name /
 * d->chanid); NULL = 'A' + channel % 26.  Either output may be left out (nmea_len == NULL /
 * text_len == NULL); a NULL buffer with a non-NULL length only sizes. */
int  gnuais_messages_from_frames(const gnuais_frame *frames, int n_frames, uint8_t *seqnr,
				 const char *chanid, int n_channels, char *nmea, size_t nmea_cap,
				 size_t *nmea_len, int *n_sentences, char *text, size_t text_cap,
				 size_t *text_len, int *n_lines);
/* The same sentences formatted ON THE DEVICE, straight from the HBM frame ring (sort into the
 * reference's order, prefix sums for the text offsets and the per-channel sequence digit, one
 * thread per frame): consumes the queued frames like gnuais_batch_drain_frames() and copies only
 * the text to the host.  Byte-identical to gnuais_nmea_from_frames() over the drained records.
 * seqnr[n_channels] in/out as there.  GNUAIS_E_ARG if `out_cap` is too small (nothing consumed;
 * 164 bytes per pending frame always suffice). */
int  gnuais_batch_drain_nmea(gnuais_batch *b, uint8_t *seqnr, char *out, size_t out_cap,
			     size_t *out_len, int *n_sentences, int *n_frames);
/* Row f1 complete ON THE DEVICE: the sentences as above AND the stdout lines of
 * gnuais_messages_from_frames() -- "ch <id> type <t> mmsi <9 digits>:" + the fields of the per-type
 * decoders (src/protodec.c:357-776) + " (!<last sentence>)\n" -- one thread per frame, printf's %.6f /
 * %.1f / %.0f done exactly in integer arithmetic; only the two texts cross PCIe.  Consumes the queued
 * frames like gnuais_batch_drain_frames().  Byte-identical to the host formatter over the drained
 * records.  chanid[n_channels] or NULL as there.  GNUAIS_E_ARG (nothing consumed) unless nmea_cap >=
 * 164 and text_cap >= 512 bytes per pending frame (gnuais_batch_pending_frames). */
int  gnuais_batch_drain_messages(gnuais_batch *b, uint8_t *seqnr, const char *chanid, char *nmea,
				 size_t nmea_cap, size_t *nmea_len, int *n_sentences, char *text,
				 size_t text_cap, size_t *text_len, int *n_lines, int *n_frames);
/* Row f3 ON THE DEVICE: gnuais_vessels_from_frames() over the queued frames without draining them -- the
 * batch's position-cache entries (one gnuais_vessel per MMSI seen, sorted by MMSI, exactly what the
 * per-type decoders' cache_*() calls leave for a fresh cache), folded by a sort on (MMSI, arrival order)
 * and one thread per vessel.  Call it before the drain that consumes the frames.  *n_vessels = entries;
 * GNUAIS_E_OVERFLOW (with *n_vessels set) if cap is too small. */
int  gnuais_batch_fold_vessels(gnuais_batch *b, gnuais_vessel *vessels, int cap, int *n_vessels);
/* Row f3, CARRIED: the reference keeps one position cache for the whole run (src/cache.c:163-384) and every
 * decoder call updates it; this is that cache kept in device memory from batch to batch.
 * gnuais_batch_vessel_table_enable(capacity) makes an empty table for `capacity` vessels (a hash table keyed by MMSI,
 * twice as many slots).  From then on every gnuais_batch_stream_nmea() call also folds the frames it takes off
 * into the table, queued behind their formatter (two small kernels, no sort, nothing waited for).  A drain-type
 * caller calls gnuais_batch_vessel_table_update() before the drain that consumes the frames: the queued
 * frames are folded (and stay queued); once per span of frames, or a frame is applied twice (harmless for the
 * result: the fold is idempotent per span).  gnuais_batch_vessel_table() waits for what has been queued and
 * returns the entries sorted by MMSI: byte for byte what gnuais_vessels_from_frames() leaves when it is fed the
 * same spans one after another.  GNUAIS_E_OVERFLOW (with *n_vessels set) when `cap` is too small or more vessels
 * were seen than the table was enabled for.  _clear() empties the table. */
int  gnuais_batch_vessel_table_enable(gnuais_batch *b, int capacity);
int  gnuais_batch_vessel_table_update(gnuais_batch *b);
int  gnuais_batch_vessel_table(gnuais_batch *b, gnuais_vessel *vessels, int cap, int *n_vessels);
int  gnuais_batch_vessel_table_clear(gnuais_batch *b);
/* Streaming delivery of the same sentences.  Call once after every gnuais_batch_run(): the frames of
 * the runs since the previous call are taken off at once (the chain moves on to another frame ring);
 * their formatter and the copy of the text into pinned host memory are queued behind the chain with every
 * size taken on the device, so the call itself waits for nothing it has queued.  *text / *len: the
 * sentences of the call D calls ago, D = gnuais_batch_info(b, "stream_depth", &D) (7: a call takes about
 * five call periods from its first kernel to its text on the host); valid until the next call;
 * *n_frames = -1 while the pipeline fills.  The per-channel sequence digit is carried on the device.
 * Calls without runs in between flush what is in flight.  Errors of a call (ring overflow, watchdog)
 * are reported when its text is handed out.  Not to be mixed with the gnuais_batch_drain_*() calls on
 * one batch. */
int  gnuais_batch_stream_nmea(gnuais_batch *b, const char **text, size_t *len, int *n_sentences,
			      int *n_frames);
/* both at once: the records (for the host-side consumers: stdout text, vessel table, range) and the
 * device-formatted sentences (for serial / IPC) of the same drained span */
int  gnuais_batch_drain_frames_nmea(gnuais_batch *b, gnuais_frame *h_frames, int max, int *n_frames,
				    uint8_t *seqnr, char *out, size_t out_cap, size_t *out_len,
				    int *n_sentences);
/* Range statistics (range.c:32-45, called from the position decoders protodec.c:399,441,628):
 * best_range_km[channel] = max(itself, great-circle km from the station to every plausible
 * position in frames of type 1-3, 4 and 18), the reference's float arithmetic step for step.
 * A station position outside (-90,90) x (-180,180) degrees means "no location" as in
 * cfg.c:364 and leaves the array untouched.  log_range() (range.c:47-53) is the caller's:
 * print entries > 0.1 and zero them. */
int  gnuais_range_from_frames(const gnuais_frame *frames, int n_frames, int n_channels,
			      float my_lat_deg, float my_lon_deg, float *best_range_km);
/* The batched front of the reference's position cache (row f3).  Folds the frames, in order,
 * into `vessels` exactly as the reference's decoders fold them into its cache one
 * cache_*() call at a time (protodec.c:282,390,435,516,619,676-678,740,772): on entry
 * `*n_vessels` entries sorted by MMSI (0 = empty cache), on return the updated table, sorted.
 * A consumer then makes one sink call per vessel and batch instead of one per message.
 * GNUAIS_E_OVERFLOW when more than `cap` vessels are needed (table left as on entry). */
int  gnuais_vessels_from_frames(const gnuais_frame *frames, int n_frames, gnuais_vessel *vessels,
				int cap, int *n_vessels);
/* benchmark input builder: d_out[l][c] = d_base[c % n_base][(l + (c * 7919) % len) % len] */
int  gnuais_tile_channels(const int16_t *d_base, int n_base, int len, int16_t *d_out,
			  int n_channels, void *stream);
/* per-kernel timing of the last run (HIP events recorded on the stream each
 * kernel is launched on), ms[5]: [0] K1 fir_slice  [1] K2 pll  [2] K2b hdlc_deframe
 * [3] K3 hdlc_crc  [4] whole call.  Needs gnuais_batch_set_timing(b, 1) before the run. */
int  gnuais_batch_set_timing(gnuais_batch *b, int on);
int  gnuais_batch_last_timing(gnuais_batch *b, float *ms5);
/* mean over the (up to 64) most recent timed runs since set_timing(b, 1); with the
 * stage pipeline on, these are the durations WHILE the stages of neighbouring
 * calls overlap */
int  gnuais_batch_mean_timing(gnuais_batch *b, float *ms5, int *n_calls);
/* Options (every setting is bit-exact):
 *   "pipeline"      1 (default): every stage on its own stream, the stages of consecutive calls overlap; 0: one stream
 *   "nbuf"          hand-off sets in use = calls that may be in flight, 2..8 (default 3; more are allocated on demand)
 *   "fir_T"         outputs per wave in K1 (multiple of 32; default 512)
 *   "fir_variant"   3 = the sign-exact slicer (default where the table allows); 0 = the exact ordered sum for every sample
 *   "fir_mfma"      long tables (192 kHz), whole groups of 64 channels, calls longer than a segment: 1 = every segment but a call's
 *                   first runs its 48 central taps as an exact integer Toeplitz product on the matrix pipe (default), 0 = packed kernel only
 *   "fir_pk_taps"   long tables (192 kHz): 0 = 40 central taps where the table's bound allows (default), 48 = 48 of them
 *   "fir_flag2"     1 = the slicer reads sign and threshold of an output off one scaled sum (default); 0 = subtract + two gathers
 *   "pll_variant"   0 = by channel count (default: the time-parallel form, pll_tp.hip, up to 1536 channels; pll_h3.hip above);
 *                   7 / 8 force one
 *   "hdlc_variant"  1 = the event-driven deframer (default); 0 = the bit-serial one
 *   "hdlc_lpw"      channels per deframer wave, 1..64 (default by channel count: as few as keep the launch at <= 512 waves --
 *                   1, 2, 4, 8 or 16 -- up to 1536 channels, 16 up to 8192, 64 where the batch fills the chip)
 *   "streaming"     0 leaves the streamed delivery (gnuais_batch_stream_nmea switches it on)
 *   "unique_hash_bits" bits of the duplicate merge's hash in use, 1..64 (default 64); tests force hash collisions with few
 *   "timing_stride" with set_timing on, time every n-th call only (the event records of a timed call cost stream time)
 *   "stage_mask"    measurement only: bit 0 FIR/slicer, 1 PLL/NRZI, 3 deframer, 4 unstuff/CRC; results are wrong unless 0x1f */
int  gnuais_batch_set_option(gnuais_batch *b, const char *name, int value);
/* Optional, once, before real work, for processes that created HIP streams of their own before the batch: time the
 * stage -> stream assignments on `d_samples` (about 1.3 s of pipelined calls: two greedy searches and a longer
 * head-to-head with the default) and keep a searched assignment only if it beats the default by 3 % or more; RESETS the
 * batch.  Which hardware queue a stream gets depends on what else the process created before, is not queryable, and
 * matters by up to 1.7x; in a process without streams of its own the default assignment (the creation order inside
 * gnuais_batch_create) is the best one found on every box measured (bench.py reports both: uncalibrated_ms_per_step). */
int  gnuais_batch_autotune(gnuais_batch *b, const int16_t *d_samples, int len, void *stream,
			   float *ms_per_call);
/* The same for the delivery loop (gnuais_batch_run + gnuais_batch_stream_nmea): places the stream of the
 * kernel that copies the text to pinned memory (one more tenant for the few hardware queues: 0.62 or 1.5 ms
 * per C3 call, by luck of creation order, unless measured).  Call it after gnuais_batch_autotune(), once,
 * before real work; about 0.2 s; RESETS the batch and leaves it in streaming mode. */
int  gnuais_batch_autotune_delivery(gnuais_batch *b, const int16_t *d_samples, int len, void *stream,
				    float *ms_per_call);
const char *gnuais_last_error(void);
const char *gnuais_version(void);

/* ---- the MySQL sink behind a batch (src/out_mysql.c:174-297, called from src/protodec.c:383,430,510,612,670,737,768,891) ----
 * What a myout_ais_*() call does depends on the reference's mysql_keepsmall (src/out_mysql.c:133-166, cfg.h:80):
 *   keepsmall on : "UPDATE <table> SET <this call's columns> WHERE mmsi", INSERT only if no row was touched -- per
 *                  table and vessel only the LAST call of each kind leaves anything in the database;
 *   keepsmall off: (the reference's default, cfg.c:74) every call INSERTs a row of its own -- nothing may be dropped.
 * gnuais_sql_calls_from_frames() walks a batch of frame records in arrival order and returns the calls to make -- kind,
 * mmsi and the argument values the reference's decoders would pass, bit for bit: with keepsmall != 0 the surviving
 * calls in their original relative order (the same final rows with <= 5 statements per vessel and batch instead of one
 * or two per message), with keepsmall == 0 every call.  gnuais_sql_plan_from_frames() is the keepsmall != 0 form.
 * (The per-sentence myout_nmea() log rows are never reduced: one per sentence of gnuais_nmea_from_frames().)  Host code. */
#define GNUAIS_SQL_POSITION    1   /* myout_ais_position(my, t, mmsi, lat, lon, hdg, course, sog)            types 1-3, 18 */
#define GNUAIS_SQL_BASESTATION 2   /* myout_ais_basestation(my, t, mmsi, lat, lon)                            type 4        */
#define GNUAIS_SQL_VESSELDATA  3   /* myout_ais_vesseldata(my, t, mmsi, name, destination, draught, A, B, C, D) type 5      */
#define GNUAIS_SQL_VESSELDATAB 4   /* myout_ais_vesseldatab(my, t, mmsi, A, B, C, D)                          types 19, 24B */
#define GNUAIS_SQL_VESSELNAME  5   /* myout_ais_vesselname(my, t, mmsi, name, destination)                    types 19, 24A */
typedef struct gnuais_sql_call {
	int32_t kind, mmsi;
	float   lat, lon, hdg, course, sog, draught;
	int32_t A, B, C, D;
	char    name[24], destination[24];
} gnuais_sql_call;
int  gnuais_sql_calls_from_frames(const gnuais_frame *frames, int n_frames, int keepsmall, gnuais_sql_call *out,
				  int cap, int *n_out);
int  gnuais_sql_plan_from_frames(const gnuais_frame *frames, int n_frames, gnuais_sql_call *out, int cap, int *n_out);

/* ---- the receivers of one NODE: N channels over several GPUs (src/ais.c:141-147, 237-247) ----------
 * gnuais creates its receivers one by one and they share nothing; the main loop hands every receiver the same
 * interleaved buffer.  A node is that over the node's devices: device g owns the contiguous channel block
 * [g*N/G, (g+1)*N/G) as a gnuais_batch of its own, one host thread per device issues that device's copies and
 * launches, nothing is exchanged between devices (no collective).  Results are merged on the host: frame records
 * carry GLOBAL channel numbers and come in the reference's order (channel, then time).
 * devices / n_devices: HIP device indices, one shard each (an index may repeat: several shards on one device);
 *   NULL / 0 = every visible device.  The other arguments as gnuais_batch_create(), per shard. */
typedef struct gnuais_node gnuais_node;
int  gnuais_node_create(gnuais_node **out, const int *devices, int n_devices, int n_channels, const float *taps,
			int n_taps, unsigned pllinc, int max_len, int frame_capacity_per_device);
void gnuais_node_destroy(gnuais_node *nd);
int  gnuais_node_reset(gnuais_node *nd);
int  gnuais_node_n_devices(const gnuais_node *nd);      /* shards */
int  gnuais_node_n_channels(const gnuais_node *nd);
/* shard i: its device, first global channel, channel count and batch (for the per-batch calls above) */
int  gnuais_node_shard(const gnuais_node *nd, int i, int *device, int *first_channel, int *n_channels,
		       gnuais_batch **batch);
/* receiver_run() for all N channels from ONE host buffer, interleaved int16 [len][N] as src/ais.c:216 holds it:
 * every device's thread copies its columns (a strided 2-D copy) and queues its chain; the call returns when
 * the buffer may be reused.  Results after gnuais_node_sync(). */
int  gnuais_node_run_host(gnuais_node *nd, const int16_t *h_samples, int len);
/* the same with the samples already on the devices: d_samples[i] = shard i's DEVICE slab, interleaved
 * int16 [len][n_channels of shard i]; streams[i] (or NULL) as in gnuais_batch_run().  Asynchronous. */
int  gnuais_node_run(gnuais_node *nd, const int16_t *const *d_samples, int len, void *const *streams);
/* complex baseband in (gnuais_batch_run_iq): one HOST buffer int16 [len][N][2]; every shard copies its columns (a 2-D
 * copy, 4 bytes per channel) and runs discriminator and chain; returns when the buffer may be reused */
int  gnuais_node_run_iq_host(gnuais_node *nd, const int16_t *h_iq, int len);
/* the same with the pairs already on the devices: d_iq[i] = shard i's DEVICE slab int16 [len][n_channels of shard i][2] */
int  gnuais_node_run_iq(gnuais_node *nd, const int16_t *const *d_iq, int len, void *const *streams);
/* wideband in at a rational ratio (gnuais_batch_resampler): configures every shard, under gnuais_node_channeliser's rule;
 * the node's wideband run calls then take len a multiple of down with len * up / down <= max_len */
int  gnuais_node_resampler(gnuais_node *nd, int up, int down, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                           const int16_t *taps, int n_taps);
/* wideband in (gnuais_batch_channeliser): configures every shard; a shard whose first channel or channel count is not a
 * multiple of n_offsets is GNUAIS_E_ARG (the message names it) */
int  gnuais_node_channeliser(gnuais_node *nd, int decim, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                             const int16_t *taps, int n_taps);
/* one HOST buffer int16 [len][N/K][2] of wide streams; every shard copies the columns of its own streams,
 * [first/K, (first+n)/K), and runs channeliser, discriminator and chain; returns when the buffer may be reused */
int  gnuais_node_run_wideband_host(gnuais_node *nd, const int16_t *h_wide, int len);
/* the same on wide samples of format fmt (GNUAIS_FMT_*), split and copied in their native bytes */
int  gnuais_node_run_wideband_fmt_host(gnuais_node *nd, int fmt, const void *h_wide, int len);
/* gnuais_batch_afc() on every shard */
int  gnuais_node_afc(gnuais_node *nd, int window);
int  gnuais_node_sync(gnuais_node *nd);
/* merged results: records of every device, channel = global index, reference order (channel, then time) */
int  gnuais_node_pending_frames(gnuais_node *nd, int *n_out);
int  gnuais_node_drain_frames(gnuais_node *nd, gnuais_frame *h_out, int max, int *n_out);
/* the frames' receive times (gnuais_batch_frame_times) on every shard, and the merged drain with them: h_times[i]
 * belongs to h_out[i]; global channel numbers and the reference's order as gnuais_node_drain_frames */
int  gnuais_node_frame_times(gnuais_node *nd, int on);
int  gnuais_node_drain_frames_timed(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out);
/* gnuais_batch_frame_signal() on every shard, and the merged drain with every record's power and carrier error */
int  gnuais_node_frame_signal(gnuais_node *nd, int on);
int  gnuais_node_drain_frames_signal(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, gnuais_frame_signal *h_signal,
                                     int max, int *n_out);
/* gnuais_batch_occupancy() on every shard, and the merged drain: the shards see the same rows, so their epochs align;
 * h_out[i][c] is the record of GLOBAL channel c.  Every shard delivers the same number of epochs (at most max) with the
 * same first blocks; GNUAIS_E_STATE if they disagree. */
int  gnuais_node_occupancy(gnuais_node *nd, int epoch_blocks, int margin);
int  gnuais_node_drain_occupancy(gnuais_node *nd, gnuais_occupancy *h_out /* [max][n_channels] */,
                                 int64_t *h_first_block /* [max] */, int max, int *n_out);
/* gnuais_batch_repair() on every shard, and the repairs per global channel */
/* gnuais_batch_long_frames / _long_counters on every shard; the drain merged over the shards, with global channel numbers,
 * in (channel, stamp) order */
int  gnuais_node_long_frames(gnuais_node *nd, int on);
int  gnuais_node_drain_long_frames(gnuais_node *nd, gnuais_long_frame *h_out, int max, int *n_out);
/* gnuais_batch_long_frame_signal() on every shard, and the long drain with every record's power and carrier error;
 * gnuais_node_drain_long_frames_heard() carries the records in its members while the feature is on */
int  gnuais_node_long_frame_signal(gnuais_node *nd, int on);
int  gnuais_node_drain_long_frames_signal(gnuais_node *nd, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max,
                                          int *n_out);
int  gnuais_node_long_counters(gnuais_node *nd, int32_t *h_delivered /* [n_channels] */, int32_t *h_failed /* [n_channels] */);
/* gnuais_batch_long_repair() on every shard, and the long frames repaired per global channel */
int  gnuais_node_long_repair(gnuais_node *nd, int on);
int  gnuais_node_long_repaired(gnuais_node *nd, int32_t *h_out /* [n_channels] */);
int  gnuais_node_repair(gnuais_node *nd, int on);
int  gnuais_node_repaired(gnuais_node *nd, int32_t *h_out /* [n_channels] */);
/* gnuais_batch_unique()'s definition over the whole node.  Copies on different shards must merge, and the shards
 * exchange nothing (no collective): so the node form is gnuais_node_drain_frames_timed() into a host buffer followed by
 * one gnuais_uniq kept in the node -- the merge itself runs on the host here, not on the devices.  _unique() needs
 * gnuais_node_frame_times on (else GNUAIS_E_STATE), which then cannot be switched off; gnuais_node_reset() clears the
 * tail and `late`.  The shards' own gnuais_batch_unique stays off. */
int  gnuais_node_unique(gnuais_node *nd, int window_rows);
int  gnuais_node_drain_frames_unique(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                     int *n_out);
int  gnuais_node_unique_late(gnuais_node *nd, long long *late);
/* gnuais_batch_drain_frames_heard()'s definition over the whole node, through the same gnuais_uniq and the same carried
 * state as gnuais_node_drain_frames_unique(); the two may be mixed.  The host merge is fed by the shards' signal drain,
 * or by their timed drain with zero records while their gnuais_batch_frame_signal is off.  Channel numbers are global. */
int  gnuais_node_drain_frames_heard(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                    int *n_out, int32_t *h_first /* [max + 1] */, gnuais_hearer *h_members /* [max] */,
                                    int *n_members);
/* gnuais_batch_long_unique()'s definition over the whole node, as gnuais_node_unique does it for the chain's frames: the
 * shards' plain long drains (gnuais_node_drain_long_frames) into a host buffer, then one gnuais_long_uniq kept in the
 * node, with the node's rows.  _long_unique() needs gnuais_node_long_frames on (else GNUAIS_E_STATE); switching that
 * switches this off; gnuais_node_reset() clears the tail and `late`.  The shards' own gnuais_batch_long_unique stays
 * off.  The two drains share the carried state and may be mixed.  Channel numbers are global. */
int  gnuais_node_long_unique(gnuais_node *nd, int window_rows);
int  gnuais_node_drain_long_frames_unique(gnuais_node *nd, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out);
int  gnuais_node_drain_long_frames_heard(gnuais_node *nd, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out,
                                         int32_t *h_first /* [max + 1] */, gnuais_hearer *h_members /* [max] */,
                                         int *n_members);
int  gnuais_node_long_unique_late(gnuais_node *nd, long long *late);
/* gnuais_batch_stream_nmea() on every shard (each from its own thread): texts[g] / lens[g] = shard g's sentences of
 * the call `stream_depth` calls ago (n_devices entries; valid until the next call).  Written out in shard order they
 * are the node's sentences in the reference's order for that call: shard g's channels all lie before shard g+1's and
 * a sentence does not name its channel.  *n_frames = -1 while the pipelines fill, else the total. */
int  gnuais_node_stream_nmea(gnuais_node *nd, const char **texts, size_t *lens, int *n_sentences, int *n_frames);
int  gnuais_node_discard_frames(gnuais_node *nd);
int  gnuais_node_counters(gnuais_node *nd, gnuais_counters *h_out /* [n_channels] */);
int  gnuais_node_total_received(gnuais_node *nd, long long *total);
int  gnuais_node_maxval(gnuais_node *nd, int16_t *h_out /* [n_channels] */);
int  gnuais_node_pll_state(gnuais_node *nd, gnuais_pll_state *h_out /* [n_channels] */);
int  gnuais_node_set_option(gnuais_node *nd, const char *name, int value);      /* on every shard */
/* gnuais_batch_autotune() on every shard, one after the other; *best_ms_max = the slowest shard's best */
int  gnuais_node_autotune(gnuais_node *nd, const int16_t *const *d_samples, int len, void *const *streams,
			  float *best_ms_max);
const char *gnuais_node_last_error(void);   /* of the calling thread: which device failed and why */
/* what gnuais_node_create() could not do without failing, one line per shard ("" when nothing): a shard's host thread that
 * could not be pinned to its device's NUMA node.  gnuais_node_create itself fails -- with the device and both figures in
 * gnuais_node_last_error() -- for a device index that is not visible and for a shard that does not fit its device's free memory. */
const char *gnuais_node_warnings(const gnuais_node *nd);
/* Where a shard runs and how it fared, for whoever times a node (a slow device must show by itself): every shard's
 * host thread is pinned, when it starts, to the CPUs of the NUMA node its device hangs off (the device's PCI address
 * -> /sys/bus/pci/devices/<addr>/numa_node -> /sys/devices/system/node/node<n>/cpulist, intersected with what the
 * process may use; GNUAIS_NODE_PIN=0 leaves the threads alone), so that what it allocates from then on -- the batch's
 * pinned staging buffers among it -- is local to that device.  gnuais_node_mark() starts a measurement;
 * after a gnuais_node_sync(), shard i reports: calls since the mark, submit_ms = host time inside its run calls,
 * busy_ms = from its first submission to the end of its own sync. */
typedef struct gnuais_node_shard_stat {
	int32_t device, first_channel, n_channels;
	int32_t numa_node;      /* -1: unknown */
	int32_t pinned_cpus;    /* 0: not pinned */
	long long calls;
	double  submit_ms, busy_ms;
	char    pci[32];
} gnuais_node_shard_stat;
int  gnuais_node_mark(gnuais_node *nd);
int  gnuais_node_shard_stats(const gnuais_node *nd, int i, gnuais_node_shard_stat *out);

#ifdef __cplusplus
}
#endif
#endif
