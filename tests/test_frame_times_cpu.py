"""The frames' receive times on the CPU: the definition (tests/frame_time_ref.py) against the true slicing row, the
generator's slots, the TAG-block formatter and the time map's arithmetic.  No GPU: the formatter is host code inside
libgnuais_hip.so and also runs here under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afc_ref
import cases
import chan_ref
import frame_time_ref as ftr
import iq_ref
from gnuais_amd import params, synth
from oracle_lib import FRAME_DTYPE, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [1, 777, 2047, 2049, 4096, 1, 6000, 2048, 333]


def calls_of(total, pattern=RAGGED):
    out, pos, i = [], 0, 0
    while pos < total:
        n = min(pattern[i % len(pattern)], total - pos)
        out.append(n)
        pos += n
        i += 1
    return out


def accuracy_inputs():
    """the inputs of DESIGN.md 4.11's table: (name, rate, samples [n])"""
    n48, n192 = 30 * synth.SLOT_BITS * 5, 8 * synth.SLOT_BITS * 20
    for seed in (1, 2, 3, 9):
        for sigma in (1000.0, 3000.0, 6000.0):
            yield f"48k seed {seed} sigma {sigma:.0f}", "48k", synth.make_stream(n48, seed=seed, sigma=sigma, occupancy=0.8)[0]
    yield "48k noise", "48k", np.rint(np.random.default_rng(5).normal(0, 3000, n48)).astype(np.int16)
    yield "48k silence", "48k", np.zeros(n48, dtype=np.int16)
    yield "192k seed 7", "192k", synth.make_stream(n192, seed=7, sps=20, occupancy=0.8)[0]
    yield "192k noise", "192k", np.rint(np.random.default_rng(6).normal(0, 3000, n192)).astype(np.int16)


@pytest.mark.parametrize("name,rate,x", list(accuracy_inputs()), ids=[a[0].replace(" ", "_") for a in accuracy_inputs()])
def test_interpolated_time_is_within_one_bit_of_the_slicing_row(name, rate, x):
    """every bit, not only frame ends: |t - true slicing row| <= ceil(65536 / pllinc) over ragged calls; the per-sample
    transcription's bit count equals the oracle's, segment by segment"""
    taps, pllinc = (None, 0x10000 // 5) if rate == "48k" else (params.taps_192k(), params.PLLINC_192K)
    bound = -(-65536 // pllinc)
    o = Oracle(1, taps, pllinc)
    state, n0 = None, 0
    errs = []
    for length in calls_of(len(x)):
        call_rows = []
        for s0 in range(0, length, ftr.SEG):
            seg = x[n0 + s0:n0 + min(s0 + ftr.SEG, length), None]
            r = o.run(seg, want_filtered=True, want_bits=True)
            rows, state = ftr.pll_rows((r["filtered"][:, 0] > 0).astype(np.uint8), pllinc, state)
            assert len(rows) == len(r["bits"][0]), (name, n0, s0)
            call_rows.append(rows + n0 + s0)
        true = np.concatenate(call_rows)
        errs.append(ftr.interp_rows(true, n0, length) - true)
        n0 += length
    err = np.concatenate(errs)                                  # by bit index since reset: a frame's stamp indexes it
    n_bits, lo, hi = len(err), int(err.min()), int(err.max())
    ends = err[ftr.stamp(o.frames())]
    at_ends = f"{int(ends.min()):+d} .. {int(ends.max()):+d} at {len(ends)} frame ends" if len(ends) else "no frames"
    print(f"{name}: {n_bits} bits, error {lo:+d} .. {hi:+d} rows ({at_ends}), bound {bound}")
    assert n_bits > len(x) * pllinc // 65536 - 64
    assert -bound <= lo and hi <= bound, (name, lo, hi, bound)


def check_slots(ref, audio_calls, placed, mul, off, slot_len):
    """run the calls; every decoded frame's mapped input time falls into the slot its payload was placed in"""
    checked = 0
    for a in audio_calls:
        ref.run(a)
        fr, times = ref.drain()
        for f, t in zip(fr, times):
            assert t >= 0
            slot = (int(t) * mul + off) // slot_len
            want = dict(placed[int(f["channel"])]).get(slot)
            assert want is not None and bytes(f["payload"][: int(f["nbits"]) // 8]) == want, (int(f["channel"]), int(t), slot)
            checked += 1
    decoded = int(ref.o.counters()[:, 0].sum())
    assert checked >= decoded and decoded > 0, (checked, decoded)
    return decoded


def test_slot_of_every_decoded_frame_audio():
    n_ch, total = 3, 40 * 1280
    made = [synth.make_stream(total, seed=4, channel=c, occupancy=0.8) for c in range(n_ch)]
    x = np.stack([m[0] for m in made], axis=1)
    cuts = np.cumsum([0] + calls_of(total))
    mul, off = ftr.time_map("audio")
    n = check_slots(ftr.FrameTimeRef(n_ch), [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [m[1] for m in made], mul, off, 1280)
    assert n > 60


@pytest.mark.parametrize("W", [0, 1024])
def test_slot_of_every_decoded_frame_iq(W):
    n_ch, total = 3, 40 * 1280
    made = [synth.make_iq_stream(total, seed=4, channel=c, sigma=800.0, occupancy=0.8, gated=True,
                                 offset_hz=3000.0 if W else 0.0) for c in range(n_ch)]
    x = np.stack([m[0] for m in made], axis=1)
    cuts = np.cumsum([0] + calls_of(total))
    afc, carry, audio = (afc_ref.Afc(n_ch, W) if W else None), None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if afc:
            audio.append(afc.apply(x[a:b]))
        else:
            y, carry = iq_ref.discriminate(x[a:b], carry)
            audio.append(y)
    mul, off = ftr.time_map("iq", afc_window=W)
    n = check_slots(ftr.FrameTimeRef(n_ch), audio, [m[1] for m in made], mul, off, 1280)
    assert n > 60


@pytest.mark.parametrize("W", [0, 1024])
def test_slot_of_every_decoded_frame_wideband(W):
    M, D, offsets = 2, 6, (-25000, 25000)
    total = 24 * 1280 * D
    made = [synth.make_wideband_stream(total, D, 48000 * D, offsets, seed=3, stream=s, sigma=500.0, occupancy=0.8, gated=True,
                                       offset_hz=2500.0 if W else 0.0) for s in range(M)]
    x = np.stack([m[0] for m in made], axis=1)
    placed = [p for m in made for p in m[1]]                # receiver s*K + k
    ch = chan_ref.Channeliser(M, D, 48000 * D, offsets)
    cuts = np.cumsum([0] + [D * n for n in calls_of(total // D)])
    afc, carry, audio = (afc_ref.Afc(M * len(offsets), W) if W else None), None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        iq = ch.run(x[a:b])
        if afc:
            audio.append(afc.apply(iq))
        else:
            y, carry = iq_ref.discriminate(iq, carry)
            audio.append(y)
    mul, off = ftr.time_map("wideband", afc_window=W, decim=D, chan_taps=16 * D + 1)
    n = check_slots(ftr.FrameTimeRef(M * len(offsets)), audio, placed, mul, off, 1280 * D)
    assert n > 40


def test_time_map_arithmetic():
    assert ftr.time_map("audio") == (1, -18)
    assert ftr.time_map("audio", n_taps=144) == (1, -72)
    assert ftr.time_map("audio", n_taps=35) == (1, -18)
    assert ftr.time_map("iq") == (1, -18) and ftr.time_map("iq", afc_window=2048) == (1, -18 - 1024)
    assert ftr.time_map("wideband", decim=6, chan_taps=97) == (6, -18 * 6 + 5 - 48)
    assert ftr.time_map("wideband", afc_window=1024, decim=6, chan_taps=97) == (6, (-18 - 512) * 6 + 5 - 48)
    assert ftr.time_map("wideband", n_taps=144, afc_window=8192, decim=4, chan_taps=65) == (4, (-72 - 4096) * 4 + 3 - 32)


def test_reference_decode_bits_and_protodec_reset():
    """the restatement itself: bits without samples give -1, protodec_reset keeps rows and bits, reset zeroes them"""
    x, _ = synth.make_stream(6 * 1280, seed=2, occupancy=1.0)
    ref = ftr.FrameTimeRef(1)
    ref.run(x[:3000, None])
    fr, t = ref.drain()
    assert len(fr) >= 1 and np.all(t >= 0) and np.all(np.diff(t) > 0) and t.max() < 3000
    bits = Oracle(1).run(x[:, None], want_bits=True)["bits"][0]
    ref.decode_bits([bits])
    fr2, t2 = ref.drain()
    assert len(fr2) >= 4 and np.all(t2 == -1)
    ref.protodec_reset()
    ref.run(x[3000:, None])
    fr3, t3 = ref.drain()
    assert len(fr3) >= 1 and t3.min() >= 3000 and np.all(ftr.stamp(fr3) > len(bits))
    ref.reset()
    ref.run(x[:3000, None])
    fr4, t4 = ref.drain()
    assert fr4.tobytes() == fr.tobytes() and np.array_equal(t4, t)


# ---- the TAG-block formatter -------------------------------------------------------------------------------------
TAG = re.compile(rb"\\c:(-?\d+)\*([0-9A-F]{2})\\")


def tagged(lib, fr, times, seq, mul, off, rate, epoch, cap=None):
    cap = 230 * max(1, len(fr)) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    need, ns = C.c_size_t(0), C.c_int(0)
    rc = lib.gnuais_nmea_tagged_from_frames(fr.ctypes.data, times.ctypes.data, len(fr), seq.ctypes.data, len(seq), mul, off, rate,
                                            epoch, out.ctypes.data if cap else None, cap, C.byref(need), C.byref(ns))
    return rc, out[: min(need.value, cap)].tobytes(), need.value, ns.value


def test_tagged_formatter():
    from gnuais_amd import lib as L, nmea_from_frames, nmea_tagged_from_frames
    lib = L.load()
    fr, n_ch = cases.nmea_frames(seed=71, n_channels=5, n_random=300)
    fr = np.ascontiguousarray(fr, dtype=FRAME_DTYPE)
    rng = np.random.default_rng(71)
    times = rng.integers(0, 1 << 40, len(fr)).astype(np.int64)
    times[::7] = -1
    times[1::7] = rng.integers(0, 40, len(times[1::7]))         # with off < 0: before the epoch second
    mul, off, rate, epoch = 6, -3200, 288000, 1_700_000_000
    plain = nmea_from_frames(fr, np.zeros(n_ch, dtype=np.uint8))
    seq = np.zeros(n_ch, dtype=np.uint8)
    rc, text, need, ns = tagged(lib, fr, times, seq, mul, off, rate, epoch)
    assert rc == 0 and need == len(text) and ns == plain.count(b"\r\n")
    assert TAG.sub(b"", text) == plain                          # with the tags removed: gnuais_nmea_from_frames()
    seq_plain = np.zeros(n_ch, dtype=np.uint8)
    nmea_from_frames(fr, seq_plain)
    assert np.array_equal(seq, seq_plain)
    assert text == nmea_tagged_from_frames(fr, times, np.zeros(n_ch, dtype=np.uint8), mul, off, rate, epoch)
    # frame by frame: the tag of every sentence, its checksum, floor division, -1, two-sentence messages
    s1 = np.zeros(n_ch, dtype=np.uint8)
    pos, two, untagged, negative = 0, 0, 0, 0
    for i, t in enumerate(times):
        sent = nmea_from_frames(fr[i:i + 1], s1).split(b"\r\n")[:-1]
        two += len(sent) == 2
        for s in sent:
            if t >= 0:
                unix = epoch + (int(t) * mul + off) // rate     # Python's // floors
                negative += int(t) * mul + off < 0
                body = b"c:%d" % unix
                x = 0
                for ch in body:
                    x ^= ch
                want = b"\\" + body + b"*%02X" % x + b"\\" + s + b"\r\n"
            else:
                untagged += 1
                want = s + b"\r\n"
            assert text[pos:pos + len(want)] == want, (pos, want, text[pos:pos + len(want)])
            pos += len(want)
    assert pos == len(text) and two > 10 and untagged > 10 and negative > 10
    # sizing, a buffer too small, bad arguments
    s0 = np.zeros(n_ch, dtype=np.uint8)
    rc, _, need0, _ = tagged(lib, fr, times, s0, mul, off, rate, epoch, cap=0)
    assert rc == 0 and need0 == len(text)
    assert tagged(lib, fr, times, s0, mul, off, rate, epoch, cap=100)[0] == L.E_OVERFLOW
    assert tagged(lib, fr, times, s0, mul, off, 0, epoch)[0] == L.E_ARG
    bad = fr.copy()
    bad["channel"][3] = n_ch
    assert tagged(lib, bad, times, s0, mul, off, rate, epoch)[0] == L.E_ARG


ASAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnuais_hip.h"
/* frames.bin, times.bin -> tagged.bin; argv: dir n_channels mul off rate epoch */
static void *slurp(const char *dir, const char *name, size_t *n)
{
	char path[1024];
	snprintf(path, sizeof path, "%s/%s", dir, name);
	FILE *f = fopen(path, "rb");
	if (!f) exit(2);
	fseek(f, 0, SEEK_END);
	*n = (size_t) ftell(f);
	fseek(f, 0, SEEK_SET);
	void *p = malloc(*n ? *n : 1);
	if (fread(p, 1, *n, f) != *n) exit(2);
	fclose(f);
	return p;
}
int main(int argc, char **argv)
{
	if (argc != 7) return 2;
	size_t nf = 0, nt = 0, need = 0, need2 = 0;
	gnuais_frame *fr = (gnuais_frame *) slurp(argv[1], "frames.bin", &nf);
	int64_t *t = (int64_t *) slurp(argv[1], "times.bin", &nt);
	const int n = (int) (nf / sizeof *fr), n_ch = atoi(argv[2]);
	if ((size_t) n * 8 != nt) return 2;
	uint8_t *seq = (uint8_t *) calloc((size_t) n_ch, 1);
	int ns = 0;
	if (gnuais_nmea_tagged_from_frames(fr, t, n, seq, n_ch, atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]),
	                                   NULL, 0, &need, &ns) != GNUAIS_OK) return 3;
	char *out = (char *) malloc(need ? need : 1);          /* exactly as large as announced */
	memset(seq, 0, (size_t) n_ch);
	if (gnuais_nmea_tagged_from_frames(fr, t, n, seq, n_ch, atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]),
	                                   out, need, &need2, &ns) != GNUAIS_OK || need2 != need) return 4;
	memset(seq, 0, (size_t) n_ch);
	if (need > 8 && gnuais_nmea_tagged_from_frames(fr, t, n, seq, n_ch, atoll(argv[3]), atoll(argv[4]), atoll(argv[5]),
	                                               atoll(argv[6]), out, need - 8, &need2, &ns) != GNUAIS_E_OVERFLOW) return 5;
	char path[1024];
	snprintf(path, sizeof path, "%s/tagged.bin", argv[1]);
	FILE *f = fopen(path, "wb");
	memset(seq, 0, (size_t) n_ch);
	gnuais_nmea_tagged_from_frames(fr, t, n, seq, n_ch, atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]), out, need,
	                               &need2, &ns);
	fwrite(out, 1, need, f);
	fclose(f);
	free(out); free(seq); free(t); free(fr);
	printf("tagged: %d sentences\n", ns);
	return 0;
}
'''


def test_tagged_formatter_under_the_sanitizers(tmp_path):
    """nmea.cpp built with -fsanitize=address,undefined as the other host units are (tests/test_sanitizers.py), over
    times at both ends of int64 and products that leave it"""
    from gnuais_amd import nmea_tagged_from_frames
    (tmp_path / "main.c").write_text(ASAN_MAIN)
    exe = tmp_path / "tagged_asan.bin"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", *san, "-std=gnu11", "-Wall", *inc, "-c", str(tmp_path / "main.c"), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", *san, "-std=c++17", "-ffp-contract=off", *inc, "-c",
                           os.path.join(ROOT, "gnuais_amd", "csrc", "nmea.cpp"), "-o", str(tmp_path / "nmea.o")])
    subprocess.check_call(["g++", *san, "-o", str(exe), str(tmp_path / "main.o"), str(tmp_path / "nmea.o"), "-lpthread", "-lm"])
    fr, n_ch = cases.nmea_frames(seed=72, n_channels=4, n_random=200)
    fr = np.ascontiguousarray(fr, dtype=FRAME_DTYPE)
    times = np.random.default_rng(72).integers(0, 1 << 40, len(fr)).astype(np.int64)
    times[:4] = [np.iinfo(np.int64).max, 0, -1, 1]
    fr.tofile(tmp_path / "frames.bin")
    times.tofile(tmp_path / "times.bin")
    args = (6, -3200, 288000, 1_700_000_000)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(tmp_path), str(n_ch), *map(str, args)], capture_output=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    got = (tmp_path / "tagged.bin").read_bytes()
    assert got == nmea_tagged_from_frames(fr, times, np.zeros(n_ch, dtype=np.uint8), *args) and got.count(b"\\c:") > 200
