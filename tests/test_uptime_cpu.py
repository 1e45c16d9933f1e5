"""The clocks of a long-running receiver on the CPU (the carries at 2^31, 2^32 and 2^37; the GPU side is
tests/test_uptime_gpu.py): the restatements agree with themselves under a shift of the origin, frame_time.hip's kernel --
its own text, built for the CPU under AddressSanitizer + UndefinedBehaviorSanitizer as a program of its own -- equals
frame_time_ref.FrameTimeRef at every origin, and the library's host arithmetic (spans, the duplicate merge, the TAG
formatter) holds at rows and times above 2^32 and 2^40.  No GPU."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import deframer_cases as dc
import frame_signal_ref as fsr
import frame_time_ref as ftr
import heard_ref as hr
import hip_cpu_build
import iq_ref
import occupancy_ref as orf
import unique_ref as ur
import uptime_ref as up
from gnuais_amd import lib, synth
from oracle_lib import FRAME_DTYPE

N_CH, CALLS = 4, (5000, 5240, 5120)          # ragged segments: 2048 + 2048 + 904, 2048 + 2048 + 1144, 2048 + 2048 + 1024
PLLINC = 0x10000 // 5
SENTINEL = -7777


@functools.lru_cache(maxsize=None)
def audio():
    return np.stack([synth.make_stream(sum(CALLS), seed=41, channel=c, occupancy=1.0)[0] for c in range(N_CH)], axis=1)


@functools.lru_cache(maxsize=None)
def iq():
    x = np.stack([synth.make_iq_stream(sum(CALLS), seed=42, channel=c, amplitude=10000.0, sigma=800.0, occupancy=0.8,
                                       gated=True)[0] for c in range(N_CH)], axis=1)
    return x, iq_ref.discriminate(x, None)[0]


def cuts():
    return np.cumsum((0,) + CALLS)


@functools.lru_cache(maxsize=None)
def at_zero():
    """the time restatement at origin zero, call by call: [(frames, times, segments, fed after the call)]"""
    ref, out = ftr.FrameTimeRef(N_CH), []
    for a, e in zip(cuts()[:-1], cuts()[1:]):
        ref.run(audio()[a:e])
        segs = list(ref.segs)
        out.append(ref.drain() + (segs, ref.fed.copy()))
    assert all(np.bincount(o[0]["channel"], minlength=N_CH).min() >= 2 for o in out)
    return out


def first_stamp(call):
    """per channel, the origin-zero stamp of the first frame the call closes"""
    fr = at_zero()[call][0]
    return [int(ftr.stamp(fr[fr["channel"] == c])[0]) for c in range(N_CH)]


def bit_origins():
    """name -> bits per channel, around call 1 (the second call) of CALLS"""
    fed1 = at_zero()[1][3]
    f1 = first_stamp(1)
    return {
        "zero": [0] * N_CH,
        "below": [1000 * c for c in range(N_CH)],
        # the first frame of the call is stamped 2^32 - 1, the count after the call is beyond the carry
        "straddle32": [up.CARRY32 - 1 - e for e in f1],
        # the count after the call is exactly 2^32 on the even channels, 2^32 - 1 on the odd ones
        "exact32": [up.CARRY32 - int(fed1[c]) - (c & 1) for c in range(N_CH)],
        # end_bit near 2^37, the count after the call small: the stamp has wrapped between the two
        "straddle37": [up.CARRY37 - 1 - e for e in f1],
        # the same behind a count that has wrapped before: every high bit the deframer keeps is set
        "beyond37": [(1 << 64) - (1 << 37) + up.CARRY37 - 1 - e for e in f1],
    }


# ---- the restatements under a shift ------------------------------------------------------------------------------

@pytest.mark.parametrize("R", up.origins())
@pytest.mark.parametrize("bits", ["below", "straddle32", "exact32", "straddle37"])
def test_the_time_restatement_shifts_with_its_origin(R, bits):
    B = bit_origins()[bits]
    ref = ftr.FrameTimeRef(N_CH, rows=R, bits=B)
    for (a, e), (f0, t0, _, fed0) in zip(zip(cuts()[:-1], cuts()[1:]), at_zero()):
        ref.run(audio()[a:e])
        fr, t = ref.drain()
        assert fr.tobytes() == up.shift_frames(f0, B).tobytes() and np.array_equal(t, t0 + R)
        assert [int(v) for v in ref.fed] == [int(b) + int(f) for b, f in zip(B, fed0)] and ref.n == R + e
        # the shift moves the stamp and nothing else, by exactly bits[channel] mod 2^37
        back = fr.copy()
        back["end_bit"], back["flags"] = f0["end_bit"], f0["flags"]
        assert back.tobytes() == f0.tobytes()
        assert [(int(s) - int(s0) - B[c]) % (1 << 37) for s, s0, c in zip(ftr.stamp(fr), ftr.stamp(f0), fr["channel"])] == [0] * len(fr)
    if bits == "straddle32":            # what the origin is for: stamps on both sides of the carry inside one drain
        fr = up.shift_frames(at_zero()[1][0], B)
        assert set(np.unique(fr["flags"] >> 1 & 31)) == {0, 1} and (fr["end_bit"] == 0xffffffff).sum() == N_CH


def signal_run(R, B):
    x, a = iq()
    ref = fsr.FrameSignalRef(N_CH, rows=R, bits=B)
    occ = orf.OccupancyRef(N_CH, 4, 16)
    ref.switch_on()
    occ.reset(R)
    out, n = [], R
    for lo, hi in zip(cuts()[:-1], cuts()[1:]):
        occ.run_iq(n, x[lo:hi])
        ref.run_iq(x[lo:hi], a[lo:hi])
        n += hi - lo
        fr, t, sig = ref.drain()
        occ.add_frames(fr, t)
        out.append((fr, t, sig))
    return out, ref.sums, occ.epochs()


@pytest.mark.parametrize("R", up.origins())
def test_the_signal_and_load_restatements_shift_with_their_origin(R):
    """every origin is a multiple of 256: the blocks of 64 rows and the epochs of 4 blocks keep their phase"""
    assert R % 256 == 0
    B = bit_origins()["straddle32"]
    zero, sums0, ep0 = signal_run(0, 0)
    got, sums, ep = signal_run(R, B)
    n_sig = 0
    for (f0, t0, s0), (fr, t, sg) in zip(zero, got):
        assert fr.tobytes() == up.shift_frames(f0, B).tobytes() and np.array_equal(t, t0 + R)
        assert sg.tobytes() == s0.tobytes()
        n_sig += int((sg["blocks"] > 0).sum())
    assert n_sig >= 8 * N_CH
    nb = sum(CALLS) // 64
    assert np.array_equal(sums.blocks(R // 64, nb), sums0.blocks(0, nb)) and sums0.blocks(0, nb)[..., 0].min() > 0
    assert len(ep) == len(ep0) >= 30
    for (j0, rec0, w0), (j, rec, w) in zip(ep0, ep):
        assert j == j0 + R // 64 and rec.tobytes() == rec0.tobytes() and np.array_equal(w, w0)
    assert sum(int(r["covered"].sum()) for _, r, _ in ep) > 50


# ---- frame_time.hip's kernel on the CPU --------------------------------------------------------------------------

def kernel_case(f, N, n_seg, seg_words, length, n0, frames, ctl, segcnt, times, count=None, blocks=0):
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    assert ctl.shape == (6, N) and segcnt.shape == (N, n_seg) and len(times) == len(frames)
    np.array([N, n_seg, seg_words, length, n0, len(frames), len(frames) if count is None else count, blocks],
             dtype=np.int64).tofile(f)
    f.write(frames.tobytes())
    f.write(ctl.astype(np.uint32).tobytes())
    f.write(segcnt.astype(np.uint32).tobytes())
    f.write(np.asarray(times, dtype=np.int64).tobytes())


def ctl_words(fed):
    """[6][N]: the deframer's words with the bit count in ctl[2] (low) and ctl[5] (high, every bit kept)"""
    ctl = np.full((6, len(fed)), 0xa5a5a5a5, dtype=np.uint32)
    ctl[2] = [int(v) & 0xffffffff for v in fed]
    ctl[5] = [(int(v) >> 32) & 0xffffffff for v in fed]
    return ctl


def run_call_case(R, B):
    """the launch behind the second call of CALLS at origin (R, B): the ring holds the first call's records (stale, left
    undrained), the second call's, one of a channel the batch does not have; -> the case's parts and the times wanted"""
    ref = ftr.FrameTimeRef(N_CH, rows=R, bits=B)
    ref.run(audio()[:CALLS[0]])
    stale, _ = ref.drain()
    ref.run(audio()[CALLS[0]:CALLS[0] + CALLS[1]])
    segs = list(ref.segs)
    fed = [int(b) + int(v) for b, v in zip(B, at_zero()[1][3])]       # not reduced: B may carry bits above 2^37
    mine, t = ref.drain()
    n_seg = 4                                   # max_len 8192: one segment more than the call uses
    segcnt = np.full((N_CH, n_seg), 400, dtype=np.uint32)            # an unused segment's count is never read
    for s, (_, _, _, cnt) in enumerate(segs):
        segcnt[:, s] = cnt
    alien = stale[:1].copy()
    alien["channel"] = N_CH
    frames = np.concatenate([stale[::2], mine[: len(mine) // 2], alien, stale[1::2], mine[len(mine) // 2:]])
    want = np.concatenate([np.full(len(stale[::2]), SENTINEL), t[: len(mine) // 2], [SENTINEL],
                           np.full(len(stale[1::2]), SENTINEL), t[len(mine) // 2:]]).astype(np.int64)
    return frames, ctl_words(fed), segcnt, n_seg, want


def test_the_frame_time_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path):
    """frame_time.hip compiled for the CPU behind tests/c/hip_cpu under ASan + UBSan and run through launch_frame_times(),
    every buffer at exactly its launch size.  Per case the ring, ctl and segcnt are built from FrameTimeRef: the fed count below 2^32; straddling it
    (record stamped before the carry, ctl after it); exactly 2^32 and 2^32 - 1 after the call; straddling 2^37 (fed small,
    end_bit near 2^37) with and without high bits above the stamp's 37; n0 at every rows origin; stale records of an
    earlier call and a record of no channel, which are left alone; a ring that counted more than it holds; a grid
    smaller than the ring; and a decode_bits launch (len 0), which gives -1."""
    exe = hip_cpu_build.build("frame_time_kernel_main.cpp", tmp_path / "frame_time_kernel.bin")
    src, dst = tmp_path / "cases.bin", tmp_path / "times.bin"
    wants, names = [], []
    with open(src, "wb") as f:
        for R in [0] + up.origins():
            for name, B in bit_origins().items():
                frames, ctl, segcnt, n_seg, want = run_call_case(R, B)
                assert (want != SENTINEL).sum() >= 2 * N_CH and (want == SENTINEL).sum() >= 2 * N_CH
                assert want[want != SENTINEL].min() >= R + CALLS[0] and want.max() < R + CALLS[0] + CALLS[1]
                kernel_case(f, N_CH, n_seg, 15, CALLS[1], R + CALLS[0], frames, ctl, segcnt, np.full(len(frames), SENTINEL))
                wants.append(want)
                names.append((R, name))
        # the ring has counted more records than it holds; and 300 records on a grid of one block
        R, B = up.ROWS[1], bit_origins()["straddle32"]
        frames, ctl, segcnt, n_seg, want = run_call_case(R, B)
        kernel_case(f, N_CH, n_seg, 15, CALLS[1], R + CALLS[0], frames, ctl, segcnt, np.full(len(frames), SENTINEL),
                    count=len(frames) + 5)
        wants.append(want)
        names.append("overflowed")
        reps = -(-300 // len(frames))
        kernel_case(f, N_CH, n_seg, 15, CALLS[1], R + CALLS[0], np.tile(frames, reps), ctl, segcnt,
                    np.full(len(frames) * reps, SENTINEL), blocks=1)
        wants.append(np.tile(want, reps))
        names.append("grid stride")
        # bits without samples: every segment may hold some, the packs are full but the last
        n_seg, seg_cap = 24, 480
        streams = [np.concatenate([np.zeros(7 * c, dtype=np.uint8), dc.STREAMS["good21_twice"], dc.STREAMS["max53"]])
                   for c in range(N_CH)]
        e0 = ftr.FrameTimeRef(N_CH)
        e0.decode_bits(streams)
        f0 = e0.drain()[0]
        B = [up.CARRY32 - 1 - int(ftr.stamp(f0[f0["channel"] == c])[1]) for c in range(N_CH)]
        ref = ftr.FrameTimeRef(N_CH, rows=up.ROWS[3], bits=B)
        ref.decode_bits(streams)
        fed = [int(v) for v in ref.fed]
        frames, t = ref.drain()
        assert len(frames) == 3 * N_CH and np.all(t == -1) and set(np.unique(frames["flags"] >> 1 & 31)) == {0, 1}
        segcnt = np.zeros((N_CH, n_seg), dtype=np.uint32)
        for c, s in enumerate(streams):
            assert len(s) > seg_cap
            for k in range(-(-len(s) // seg_cap)):
                segcnt[c, k] = min(seg_cap, len(s) - k * seg_cap)
        kernel_case(f, N_CH, n_seg, 15, 0, up.ROWS[3], frames, ctl_words(fed), segcnt, np.full(len(frames), SENTINEL))
        wants.append(t)
        names.append("decode_bits")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip() == "cases: %d" % len(wants)
    got = np.fromfile(dst, dtype=np.int64)
    assert got.size == sum(len(w) for w in wants)
    pos = 0
    for name, want in zip(names, wants):
        assert np.array_equal(got[pos:pos + len(want)], want), (name, got[pos:pos + len(want)], want)
        pos += len(want)


# ---- the library's host arithmetic at large clocks ---------------------------------------------------------------

def test_spans_of_the_library_equal_the_restatement_around_every_origin():
    """gnuais_frame_signal_span and gnuais_occupancy_cover_span: t and v0 around every rows origin, +-1 and +- one block,
    every frame length class, both tables' delays and an AFC window"""
    n = 0
    for R in up.origins():
        near = [R + d for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65)]
        for v0 in near + [0]:
            for dt in (0, 1, 17, 63, 64, 500, 1279, 1280, 2560, 2561, 7680):
                for nbits in (0, 168, 424):
                    for n_taps, W in ((36, 0), (144, 1024)):
                        t = R + dt
                        assert lib.frame_signal_span(t, nbits, PLLINC, n_taps, W, v0) == fsr.span(t, nbits, PLLINC, n_taps, W, v0)
                        assert lib.occupancy_cover_span(t, nbits, PLLINC, n_taps, W, v0) == orf.cover_span(t, nbits, PLLINC, n_taps, W, v0)
                        n += fsr.span(t, nbits, PLLINC, n_taps, W, v0)[1] > 0
    assert n > 1000
    # the same span, shifted: block indices + R / 64
    for R in up.origins():
        j0, nb0 = lib.frame_signal_span(5000, 168, PLLINC, 36, 0, 0)
        assert nb0 == 14 and lib.frame_signal_span(R + 5000, 168, PLLINC, 36, 0, R) == (j0 + R // 64, nb0)
        c0, cb0 = lib.occupancy_cover_span(5000, 168, PLLINC, 36, 0, 0)
        assert cb0 > nb0 and lib.occupancy_cover_span(R + 5000, 168, PLLINC, 36, 0, R) == (c0 + R // 64, cb0)


def merge_input():
    """a few drains of timed frames with copies in and beyond the window, late copies, untimed and repaired frames"""
    rng = np.random.default_rng(9)
    pay = [rng.integers(0, 256, 53, dtype=np.uint8) for _ in range(12)]
    drains, t0 = [], 0
    for d in range(5):
        n = 120
        fr = np.zeros(n, dtype=FRAME_DTYPE)
        fr["channel"] = rng.integers(0, 9, n)
        fr["end_bit"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k = rng.integers(0, len(pay), n)
        fr["payload"] = np.stack([pay[(i - d) % len(pay)] for i in k])       # the last group's payload opens the next drain
        fr["payload"][:, 21:] = 0
        fr["nbits"] = 168
        fr["flags"] = 1 | (rng.integers(0, 32, n) << 1).astype(np.uint8) | np.where(rng.random(n) < 0.2, 0x40, 0).astype(np.uint8)
        t = t0 + 300 * k + rng.integers(0, 200, n)          # copies of a payload within ~200 rows, the next 100 further on
        t[rng.random(n) < 0.1] = -1
        t0 += 3500                                          # the next drain's first copies chain onto this one's tail
        drains.append((fr, t.astype(np.int64), t0))
    return drains


@pytest.mark.parametrize("R", [up.ROWS[1], (1 << 39) - 7000, up.ROWS[3], (1 << 62) - 256])
def test_the_duplicate_merge_above_2_to_the_32_equals_itself_at_zero_shifted(R):
    """gnuais_uniq_push and gnuais_uniq_push_heard with times and rows above 2^32, across 2^39 (where a 64-bit sort word
    of (t, 24 channel bits) runs out), above 2^40 and near 2^62 == the same pushes at origin zero with the times shifted,
    `late` included; and both == the restatement at the shifted origin"""
    from gnuais_amd import Uniq
    W = 128
    for heard in (False, True):
        u0, uR, ref = Uniq(W), Uniq(W), hr.HeardRef(W)
        late = 0
        for fr, t, rows in merge_input():
            tR = np.where(t < 0, -1, t + R)
            if heard:
                a, b, w = u0.push_heard(fr, t, rows), uR.push_heard(fr, tR, rows + R), ref.push_heard(fr, tR, rows + R)
            else:
                a, b, w = u0.push(fr, t, rows), uR.push(fr, tR, rows + R), ref.push(fr, tR, rows + R)
            assert b[0].tobytes() == a[0].tobytes() == w[0].tobytes() and len(a[0]) < len(fr)
            assert np.array_equal(b[1], np.where(a[1] < 0, -1, a[1] + R)) and np.array_equal(b[1], w[1])
            assert np.array_equal(b[2], a[2]) and np.array_equal(b[2], w[2])
            if heard:
                assert np.array_equal(b[3], a[3]) and np.array_equal(b[3], w[3])
                m = a[4].copy()
                m["t"] = np.where(m["t"] < 0, -1, m["t"] + R)
                assert b[4].tobytes() == m.tobytes() == w[4].tobytes()
            assert uR.late() == u0.late() == ref.late
            late = uR.late()
        assert late > 5


TAG = re.compile(rb"\\c:(-?\d+)\*([0-9A-F]{2})\\")


def test_the_tag_formatter_prints_every_digit_of_a_large_time():
    """gnuais_nmea_tagged_from_frames with one input sample per second, so that the tag is the time itself: times at and
    above 2^31, 2^32, 2^40 and at 2^62"""
    import cases
    from gnuais_amd import nmea_from_frames, nmea_tagged_from_frames
    fr, n_ch = cases.nmea_frames(seed=72, n_channels=3, n_random=40)
    fr = np.ascontiguousarray(fr[fr["nbits"] >= 8][:24], dtype=FRAME_DTYPE)
    edges = [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, up.ROWS[1] + 3841, (1 << 37) + 5, (1 << 40) - 1,
             1 << 40, up.ROWS[3] + 12345, (1 << 53) + 1, 1 << 62]
    times = np.array([edges[i % len(edges)] for i in range(len(fr))], dtype=np.int64)
    text = nmea_tagged_from_frames(fr, times, np.zeros(n_ch, dtype=np.uint8), 1, 0, 1, 0)
    assert TAG.sub(b"", text) == nmea_from_frames(fr, np.zeros(n_ch, dtype=np.uint8))
    seq, pos = np.zeros(n_ch, dtype=np.uint8), 0
    for i, t in enumerate(times):
        for s in nmea_from_frames(fr[i:i + 1], seq).split(b"\r\n")[:-1]:
            body = b"c:" + str(int(t)).encode()
            x = 0
            for ch in body:
                x ^= ch
            want = b"\\" + body + b"*%02X" % x + b"\\" + s + b"\r\n"
            assert text[pos:pos + len(want)] == want, (int(t), text[pos:pos + len(want)])
            pos += len(want)
    assert pos == len(text)
    # and through the time map of a real rate: floor((t * mul + off) / rate) in Python integers
    mul, off, rate, epoch = 6, -3200, 288000, 1_700_000_000
    small = times[times < (1 << 60)]
    text = nmea_tagged_from_frames(fr[: len(small)], small, np.zeros(n_ch, dtype=np.uint8), mul, off, rate, epoch)
    got = [int(m.group(1)) for m in TAG.finditer(text)]
    seq = np.zeros(n_ch, dtype=np.uint8)
    want = [epoch + (int(t) * mul + off) // rate for i, t in enumerate(small)
            for _ in nmea_from_frames(fr[i:i + 1], seq).split(b"\r\n")[:-1]]
    assert got == want and max(got) > 1 << 37
