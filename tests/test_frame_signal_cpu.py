"""The frames' signal power and carrier error on the CPU: the restatement (tests/frame_signal_ref.py) against the signal
model of the generator, the span arithmetic of the library (host code inside libgnuais_hip.so, also under
AddressSanitizer + UndefinedBehaviorSanitizer as a program of its own) against the restatement's, and the block sums'
independence of where the stream is cut.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import afc_ref
import frame_signal_ref as fsr
import iq_ref
from gnuais_amd import lib, params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 48000.0
N_ROWS = 40 * synth.SLOT_BITS * 5
# amplitude, sigma, carrier offsets (Hz), AFC window: the settings of DESIGN.md 4.15's table
SETTINGS = [(10000.0, 800.0, (0.0, 300.0, -300.0), 0), (10000.0, 1500.0, (0.0, 300.0, -300.0), 0),
            (3000.0, 500.0, (0.0, 300.0, -300.0), 0), (20000.0, 1500.0, (0.0, 300.0, -300.0), 0),
            (10000.0, 800.0, (3000.0,), 2048), (3000.0, 500.0, (-4000.0,), 2048)]
CASES = [(a, s, o, w) for a, s, offs, w in SETTINGS for o in offs]


def decode(iq, W, ref):
    """one call of I/Q [len][n_ch][2] through discriminator (and AFC) into the restatement"""
    if W:
        audio = afc_ref.Afc(iq.shape[1], W).apply(iq)
    else:
        audio, _ = iq_ref.discriminate(iq, None)
    ref.run_iq(iq, audio)


@pytest.mark.parametrize("A,sigma,offset,W", CASES)
def test_restatement_against_the_signal_model(A, sigma, offset, W):
    """blocks == 14 for every 168-bit frame, power within 5 % of A^2 + 2 sigma^2, ferr within 600 Hz of the carrier
    offset per frame and within 50 Hz in the mean"""
    ratio, err = [], []
    for seed in (4, 5, 6):
        iq = synth.make_iq_stream(N_ROWS, seed=seed, amplitude=A, sigma=sigma, occupancy=0.8, gated=True,
                                  offset_hz=offset)[0][:, None, :]
        ref = fsr.FrameSignalRef(1, afc_window=W)
        ref.switch_on()
        decode(iq, W, ref)
        fr, t, sig = ref.drain()
        assert np.all(fr["nbits"] == 168) and np.all(sig["blocks"] == 14), (fr["nbits"], sig["blocks"])
        ratio.append(sig["power"] / (A * A + 2.0 * sigma * sigma))
        err.append(lib.signal_hz(sig["ferr"], RATE) - offset)
    ratio, err = np.concatenate(ratio), np.concatenate(err)
    print(f"A {A:.0f} sigma {sigma:.0f} offset {offset:+.0f} Hz W {W}: {len(err)} frames, power ratio {ratio.min():.3f} .. "
          f"{ratio.max():.3f}, ferr - offset {err.min():+.0f} .. {err.max():+.0f} Hz, mean {err.mean():+.1f}, std {err.std():.0f}")
    assert len(err) >= 50                                   # of about 96 transmissions: enough for the mean to mean something
    assert ratio.min() >= 0.95 and ratio.max() <= 1.05
    assert np.abs(err).max() <= 600.0
    assert abs(err.mean()) <= 50.0


def span_inputs(n=20000, seed=11):
    """random (t, nbits, pllinc, n_taps, W, v0): both tables' pllinc, negative q, spans behind v0, t = -1"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-1, 200000, n)
    t[: n // 10] = rng.integers(0, 600, n // 10)            # q < 0 and q - S < 0
    t[n // 10: n // 8] = rng.integers(1 << 40, 1 << 41, n // 8 - n // 10)
    nbits = rng.choice([0, 8, 72, 168, 424, 448, 65535], n)
    pllinc = rng.choice([0x10000 // 5, params.PLLINC_192K, 4096, 1, 0xffff], n)
    n_taps = rng.choice([36, 144, 1, 1023], n)
    W = rng.integers(0, 129, n) * 128
    v0 = np.where(rng.random(n) < 0.5, 0, np.maximum(t - rng.integers(0, 20000, n), 0))
    return np.stack([t, nbits, pllinc, n_taps, W, v0], axis=1).astype(np.int64)


def test_span_of_the_library_equals_the_restatement():
    x = span_inputs()
    got = np.array([lib.frame_signal_span(*map(int, row)) for row in x], dtype=np.int64)
    want = np.array([fsr.span(*map(int, row)) for row in x], dtype=np.int64)
    assert np.array_equal(got, want), x[np.argwhere((got != want).any(axis=1))[:5, 0]]
    assert (want[:, 1] > 0).sum() > 5000 and (want[:, 1] == 0).sum() > 2000 and (want[:, 0] < 0).sum() == 0
    for bad in ((5, 168, 0, 36, 0, 0), (5, -1, 13107, 36, 0, 0), (5, 168, 0x10000, 36, 0, 0), (5, 168, 13107, 36, -128, 0)):
        with pytest.raises(lib.GnuaisError) as e:
            lib.frame_signal_span(*bad)
        assert e.value.code == lib.E_ARG


ASAN_MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "gnuais_hip.h"
/* argv[1]: int64 [n][6] = t, nbits, pllinc, n_taps, W, v0; argv[2]: int64 [n][2] = j_lo, nb out */
int main(int argc, char **argv)
{
	if (argc < 3) return 1;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	const long n = bytes / 48;
	int64_t *in = (int64_t *) malloc((size_t) bytes ? (size_t) bytes : 1), *out = (int64_t *) malloc((size_t) n * 16 + 1);
	if (fread(in, 48, (size_t) n, f) != (size_t) n) return 3;
	fclose(f);
	for (long k = 0; k < n; ++k) {
		const int64_t *r = in + 6 * k;
		long long j_lo = -7;
		int nb = -7;
		if (gnuais_frame_signal_span(r[0], (int) r[1], (unsigned) r[2], (int) r[3], (int) r[4], r[5], &j_lo, &nb) != GNUAIS_OK) return 4;
		out[2 * k] = j_lo;
		out[2 * k + 1] = nb;
	}
	if (gnuais_frame_signal_span(1, 168, 0, 36, 0, 0, &(long long){0}, &(int){0}) != GNUAIS_E_ARG) return 5;
	if (gnuais_frame_signal_span(1, 168, 13107, 36, 0, 0, NULL, NULL) != GNUAIS_E_ARG) return 6;
	f = fopen(argv[2], "wb");
	fwrite(out, 16, (size_t) n, f);
	fclose(f);
	free(in); free(out);
	printf("spans: %ld\n", n);
	return 0;
}
'''


def test_span_under_the_sanitizers(tmp_path):
    """frame_signal.cpp built with -fsanitize=address,undefined as the other host units are (tests/test_sanitizers.py),
    in a program of its own, over the same inputs and times at the far end of int64"""
    (tmp_path / "main.c").write_text(ASAN_MAIN)
    exe = tmp_path / "span_asan.bin"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", *san, "-std=gnu11", "-Wall", *inc, "-c", str(tmp_path / "main.c"), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", *san, "-std=c++17", *inc, "-c", os.path.join(ROOT, "gnuais_amd", "csrc", "frame_signal.cpp"),
                           "-o", str(tmp_path / "span.o")])
    subprocess.check_call(["g++", *san, "-o", str(exe), str(tmp_path / "main.o"), str(tmp_path / "span.o")])
    x = span_inputs(seed=12)
    x[:3, 0] = [(1 << 62), (1 << 62) - 1, 0]
    x[:3, 5] = [0, 1 << 61, 0]
    x.tofile(tmp_path / "in.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.int64).reshape(-1, 2)
    want = np.array([fsr.span(*map(int, row)) for row in x], dtype=np.int64)
    assert np.array_equal(got, want)


def edge_stream(n_ch=3, n=64 * 40 + 17, seed=3):
    """random pairs with whole blocks of (-32768, -32768), (32767, -32768) and 0: P and r at 2^31"""
    iq = np.random.default_rng(seed).integers(-32768, 32768, (n, n_ch, 2)).astype(np.int16)
    iq[64 * 3:64 * 6] = -32768
    iq[64 * 8:64 * 10, :, 0], iq[64 * 8:64 * 10, :, 1] = 32767, -32768
    iq[64 * 12:64 * 14] = 0
    return iq


def test_block_sums_do_not_depend_on_the_cuts():
    iq = edge_stream()
    n, n_ch = iq.shape[:2]
    # the whole stream, summed directly
    P, r, i = fsr.row_terms(iq, np.zeros((n_ch, 2), dtype=np.int16))
    full = n // 64 * 64
    want = np.stack([P, r, i], axis=-1)[:full].reshape(-1, 64, n_ch, 3).sum(axis=1)
    assert want[4, 0, 0] == 64 << 31 and want[4, 0, 1] == 64 << 31           # beyond int32, exact
    whole = fsr.BlockSums(n_ch)
    whole.feed(0, iq)
    assert np.array_equal(whole.blocks(0, full // 64), want)
    for cut in (1, 63, 64, 65, 777):
        s = fsr.BlockSums(n_ch)
        for lo in range(0, n, cut):
            s.feed(lo, iq[lo:lo + cut])
        assert np.array_equal(s.blk, whole.blk), cut


def test_an_audio_call_in_between_zeroes_every_frame_whose_span_reaches_behind_it():
    n_ch, rows = 2, 24 * synth.SLOT_BITS * 5
    iq = np.stack([synth.make_iq_stream(rows, seed=8, channel=c, sigma=800.0, occupancy=0.9, gated=True)[0]
                   for c in range(n_ch)], axis=1)
    audio, _ = iq_ref.discriminate(iq, None)
    a, b = 10 * 1280 + 300, 12 * 1280 + 100                 # the audio call: rows [a, b), cut inside bursts
    cut = fsr.FrameSignalRef(n_ch)
    cut.switch_on()
    cut.run_iq(iq[:a], audio[:a])
    cut.run_audio(audio[a:b])
    cut.run_iq(iq[b:], audio[b:])
    fr, t, sig = cut.drain()
    whole = fsr.FrameSignalRef(n_ch)
    whole.switch_on()
    whole.run_iq(iq, audio)
    wf, wt, wsig = whole.drain()
    assert fr.tobytes() == wf.tobytes() and len(fr) > 30
    lo = np.array([fsr.span(int(x), int(nb), 0x10000 // 5)[0] * 64 for x, nb in zip(wt, wf["nbits"])])
    hi = wt - 18                                            # q
    before, behind = hi < a, lo >= b
    touched = ~before & ~behind
    assert touched.sum() >= 2 and before.sum() > 10 and behind.sum() > 10
    assert np.all(sig[touched]["blocks"] == 0) and np.all(sig[touched]["power"] == 0) and np.all(sig[touched]["ferr"] == 0)
    assert np.array_equal(sig[before], wsig[before]) and np.all(sig[before]["blocks"] > 0)
    # behind it the run starts from the pair (0, 0) again: only a block whose first row is the run's first differs
    first_blk = -(-b // 64)
    same = behind & (lo // 64 > first_blk)
    assert np.array_equal(sig[same], wsig[same]) and same.sum() > 10
