"""Messages of three to five slots on the device (gnuais_batch_long_frames, hdlc_long.hip).  Every comparison is against
the restatement tests/long_ref.py, and every test also checks that the chain's own frames, counters, fsm_state and
pll_state are identical with the feature on and off (a twin batch gets the same calls with the feature off)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import long_ref as lr
from gnuais_amd import synth
from long_ref import SampleRef
from test_iq_gpu import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def chain_state(b):
    return (b.drain_frames().tobytes(), b.counters().tobytes(), b.fsm_state().tobytes(), b.pll_state().tobytes())


def fsm_rows(ds):
    return [d.fields() for d in ds]


def got_rows(b):
    return [tuple(int(v) for v in r) for r in b.long_fsm_state()]


def twins(n_ch, **kw):
    """(batch with the feature on, batch with it off)"""
    from gnuais_amd import ReceiverBatch
    on, off = ReceiverBatch(n_ch, **kw), ReceiverBatch(n_ch, **kw)
    assert on.info("long_frames") == 0
    on.long_frames(True)
    assert on.info("long_frames") == 1 and on.info("long_frame_cap") >= 256
    return on, off


def check(b, ds, times=None):
    """one drain and the counters against the restatement; -> the records"""
    got = b.drain_long_frames()
    want = lr.records(ds, times)
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    d, f = b.long_counters()
    assert np.array_equal(np.stack([d, f], axis=1), np.array([x.long_counters() for x in ds], dtype=np.int32))
    return got


def test_basic_delivery_two_waves_the_second_ragged():
    """decode_bits on 70 channels: per channel another order of bursts of 53 .. 127 bytes with noise between them, some
    with a flipped bit; two calls that cut the streams anywhere, one drain, D''s state after every call"""
    N = 70
    rng = np.random.default_rng(41)
    streams = [lr.channel_bits(rng, c) for c in range(N)]
    cuts = [int(rng.integers(1, s.size)) for s in streams]
    b, off = twins(N, max_len=8192)
    ds = [lr.LongDeframer() for _ in range(N)]
    for part in ([s[:k] for s, k in zip(streams, cuts)], [s[k:] for s, k in zip(streams, cuts)]):
        b.decode_bits(part)
        off.decode_bits(part)
        for d, p in zip(ds, part):
            d.feed(p)
        assert got_rows(b) == fsm_rows(ds)
    got = check(b, ds)
    assert len(got) > 100 and (got["t"] == -1).all() and {int(n) for n in got["nbits"]} == {432, 440, 480, 800, 1008}
    assert sum(d.long_counters()[1] for d in ds) > 10
    assert chain_state(b) == chain_state(off)
    assert b.pending_long_frames() == 0


def test_one_burst_cut_at_every_bit_in_two_and_in_three_calls():
    """a 126-byte burst; channel c gets its first c bits in call 1 and the rest in call 2 -- then c bits, one bit, the rest"""
    rng = np.random.default_rng(42)
    s = np.concatenate([lr.burst(rng.integers(0, 256, 126, dtype=np.uint8)), np.zeros(2, dtype=np.uint8)])
    L = s.size
    assert 1060 < L < 1110
    N = L + 1
    d = lr.LongDeframer()
    before = []
    d.feed(s, states=before)
    before.append(d.fields())                               # before[i]: the machine with i bits fed
    assert [f["n"] for f in d.long_frames()] == [1008]
    b, off = twins(N, max_len=8192)
    for plan in ((lambda c: [s[:c], s[c:]]), (lambda c: [s[:c], s[c:c + 1], s[c + 1:]])):
        parts = [plan(c) for c in range(N)]
        fed = np.zeros(N, dtype=np.int64)
        for k in range(len(parts[0])):
            call = [p[k] for p in parts]
            b.decode_bits(call)
            off.decode_bits(call)
            fed += [len(x) for x in call]
            assert got_rows(b) == [before[i] for i in fed]
        got = b.drain_long_frames()
        want = lr.records([d] * N)
        assert got.tobytes() == want.tobytes()
        assert chain_state(b) == chain_state(off)
        b.reset()
        off.reset()
        dl, fl = b.long_counters()
        assert not dl.any() and not fl.any() and b.pending_long_frames() == 0


def limit_streams():
    """channel 0: 1030 stored bits, the longest frame D' delivers; 1: one bit more, given up on the flag's fifth 1;
    2: all ones, the most stuffed zeros; 3: a long frame with one bit flipped; 4: a second frame right behind a given-up one"""
    rng = np.random.default_rng(43)
    p126 = rng.integers(0, 256, 126, dtype=np.uint8)
    full = lr.burst(p126)
    body = full[32:-8]                                      # stuffed payload + FCS
    longer = np.concatenate([full[:32], body[:200], [0], body[200:], full[-8:]]).astype(np.uint8)   # one more stored bit
    ones = lr.burst(np.full(126, 0xFF, dtype=np.uint8))
    flipped = full.copy()
    flipped[500] ^= 1
    tail = np.zeros(3, dtype=np.uint8)
    return [np.concatenate([full, tail]), np.concatenate([longer, tail]), np.concatenate([ones, tail]),
            np.concatenate([flipped, tail]), np.concatenate([longer, lr.burst(p126[:60]), tail])]


def test_the_limits_1030_delivered_1031_given_up_all_words_of_the_record():
    streams = limit_streams()
    N = len(streams)
    ds = [lr.LongDeframer() for _ in range(N)]
    at_limit, before = [], []
    for d, s in zip(ds, streams):
        st = []
        d.feed(s, states=st)
        at_limit.append(max(f[6] for f in st))
        before.append(st)
    assert at_limit[0] == 1030 and [f["n"] for f in ds[0].long_frames()] == [1008]
    assert at_limit[1] == 1030 and ds[1].closed == []       # reached 1031 inside ST_DATA: reset, nothing closed
    assert [f["n"] for f in ds[2].long_frames()] == [1008] and np.count_nonzero(streams[2] == 0) > 200
    assert ds[3].long_counters() == (0, 1) and ds[4].long_counters() == (1, 0)
    b, off = twins(N, max_len=8192)
    # the given-up case: the state right behind the bit that reached 1031, and at the end
    k = int(np.argmax([f[6] for f in before[1]])) + 1       # before[1][k - 1]: 1030 stored, bit k - 1 is the 1031st
    part1 = [s[:k] for s in streams]
    b.decode_bits(part1)
    off.decode_bits(part1)
    d1 = [lr.LongDeframer() for _ in range(N)]
    for d, p in zip(d1, part1):
        d.feed(p)
    assert d1[1].fields()[0] == 1 and d1[1].fields()[6] == 0 and got_rows(b) == fsm_rows(d1)
    part2 = [s[k:] for s in streams]
    b.decode_bits(part2)
    off.decode_bits(part2)
    assert got_rows(b) == fsm_rows(ds)
    got = check(b, ds)
    assert [int(c) for c in got["channel"]] == [0, 2, 4]
    assert chain_state(b) == chain_state(off)


def seed9(n_ch=3):
    x = synth.make_stream(6 * 8 * 1280, seed=9, sigma=500.0, payloads=lr.long_payloads())[0]
    return np.stack([np.roll(x, 1111 * c) for c in range(n_ch)], axis=1)


@pytest.mark.parametrize("variant", [0, 8])
def test_through_the_samples_ragged_calls_and_times(variant):
    x = seed9()
    b, off = twins(3, max_len=5000)
    for q in (b, off):
        q.set_option("pll_variant", variant)
    ref = SampleRef(3)
    xd = dev(x)
    a = 0
    while a < x.shape[0]:
        for n in (4096, 1, 2047, 5000):
            e = min(a + n, x.shape[0])
            if e > a:
                b.run(xd[a:e])
                off.run(xd[a:e])
                ref.run(x[a:e])
                assert got_rows(b) == fsm_rows(ref.ds)
            a = e
    got = check(b, ref.ds, ref.t)
    assert len(got) >= 14 and got["t"].min() > 0 and np.all(np.diff(got["t"][got["channel"] == 0]) > 0)
    assert chain_state(b) == chain_state(off)


def test_through_run_iq():
    total = 6 * 8 * 1280
    made = [synth.make_iq_stream(total, seed=9, channel=c, sigma=500.0, payloads=lr.long_payloads()) for c in range(2)]
    iq = np.stack([m[0] for m in made], axis=1)
    import iq_ref
    b, off = twins(2, max_len=8192)
    ref = SampleRef(2)                                      # on the restated discriminator's audio
    carry = None
    for a in range(0, total, 8192):
        part = dev(iq[a:a + 8192])
        b.run_iq(part)
        off.run_iq(part)
        audio, carry = iq_ref.discriminate(iq[a:a + 8192], carry)
        ref.run(audio)
        assert got_rows(b) == fsm_rows(ref.ds)
    got = check(b, ref.ds, ref.t)
    assert len(got) >= 8 and (got["t"] > 0).all() and (got["t"] < total).all()
    placed = {p for m in made for _, p in m[1]}
    assert all(bytes(f["payload"][: f["nbits"] // 8]) in placed for f in got)
    assert chain_state(b) == chain_state(off)


def test_clocks_switches_resets_overflow_and_streaming():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_OVERFLOW, E_STATE, GnuaisError
    rng = np.random.default_rng(44)
    N = 4
    mk = lambda nb: lr.burst(rng.integers(0, 256, nb, dtype=np.uint8))
    # switched on after 10 000 bits, in mid-burst on channel 1: stamps still equal the chain's count
    first = [mk(100) for _ in range(N)]
    lead = [np.concatenate([rng.integers(0, 2, 10000 - 300 * (c == 1), dtype=np.uint8), first[c][: 300 * (c == 1)]]) for c in range(N)]
    rest = [np.concatenate([first[c][300 * (c == 1):], rng.integers(0, 2, 50, dtype=np.uint8), mk(126), np.zeros(2, np.uint8)]) for c in range(N)]
    b = ReceiverBatch(N, max_len=8192)
    off = ReceiverBatch(N, max_len=8192)
    b.decode_bits(lead)
    off.decode_bits(lead)
    b.long_frames(True)
    ds = [lr.LongDeframer(seen=len(l)) for l in lead]
    b.decode_bits(rest)
    off.decode_bits(rest)
    for d, r in zip(ds, rest):
        d.feed(r)
    got = check(b, ds)
    assert len(got) >= 2 * N - 1 and got_rows(b) == fsm_rows(ds)        # channel 1 missed the start of its first burst
    assert chain_state(b) == chain_state(off)

    # set_clock: bit counts just below 2^32 and 2^37 (the carry into flags[5:1], the wrap), t across 2^31 rows
    x = seed9(N)[:16384]
    bits0 = np.array([(1 << 32) - 1500, (1 << 37) - 1500, (7 << 32) + 5, 0], dtype=np.uint64)
    rows0 = (1 << 31) - 9000
    for q in (b, off):
        q.reset()
        q.set_clock(rows0, bits0)
    ref = SampleRef(N, rows=rows0, bits=bits0)
    for a in range(0, x.shape[0], 8192):
        b.run(dev(x[a:a + 8192]))
        off.run(dev(x[a:a + 8192]))
        ref.run(x[a:a + 8192])
    got = b.drain_long_frames()
    want = lr.records(ref.ds, ref.t)
    assert got.tobytes() == want.tobytes() and len(got) >= 2 * N
    st = (got["flags"].astype(np.int64) >> 1 << 32) | got["end_bit"]
    assert st[got["channel"] == 0].min() < 1 << 32 <= st[got["channel"] == 0].max()
    assert st[got["channel"] == 1].min() < 3000 and st[got["channel"] == 1].max() > 1 << 36       # across the wrap
    assert got["t"].min() < 1 << 31 < got["t"].max()
    assert chain_state(b) == chain_state(off)

    # protodec_reset in the middle of a long frame: the machine starts over, the count and the counters stay
    b.reset()
    burst = mk(126)
    b.decode_bits([burst[:700]] * N)
    assert got_rows(b)[0][0] == 4
    b.protodec_reset()
    ds = [lr.LongDeframer() for _ in range(N)]
    for d in ds:
        d.feed(burst[:700])
        d.protodec_reset()
        d.feed(np.concatenate([burst[700:], burst, np.zeros(2, np.uint8)]))
    b.decode_bits([np.concatenate([burst[700:], burst, np.zeros(2, np.uint8)])] * N)
    got = check(b, ds)
    assert len(got) >= N and got_rows(b) == fsm_rows(ds)
    b.decode_bits([burst[:700]] * N)
    b.reset()                                               # reset: everything
    assert all(r == (1, 0, 0, 0, 0, 0, 0) for r in got_rows(b)) and b.pending_long_frames() == 0
    assert not b.long_counters()[0].any()

    # ring overflow: GNUAIS_E_OVERFLOW, the oldest records kept, the counters exact
    cap = int(b.info("long_frame_cap"))
    per = cap // N + 2
    one = np.concatenate([mk(54), np.zeros(2, np.uint8)])
    ds = [lr.LongDeframer() for _ in range(N)]
    for _ in range(per):
        b.decode_bits([one] * N)
        for d in ds:
            d.feed(one)
    with pytest.raises(GnuaisError) as e:
        b.drain_long_frames()
    assert e.value.code == E_OVERFLOW and len(e.value.frames) == cap
    oldest = {(int(f["channel"]), int(f["end_bit"])) for f in e.value.frames}
    assert oldest == {(c, f["end_bit"]) for c in range(N) for f in ds[c].long_frames()[: cap // N]}
    assert np.array_equal(b.long_counters()[0], np.full(N, per)) and b.pending_long_frames() == 0

    # streaming, both ways
    for call in (b.stream_nmea, lambda: b.set_option("streaming", 1)):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    b.long_frames(False)
    assert b.info("long_frames") == 0
    b.stream_nmea()
    with pytest.raises(GnuaisError) as e:
        b.long_frames(True)
    assert e.value.code == E_STATE
    b.set_option("streaming", 0)
    never = ReceiverBatch(2, max_len=4096)
    with pytest.raises(GnuaisError) as e:
        never.drain_long_frames()
    assert e.value.code == E_STATE


def test_a_node_of_two_shards_equals_one_batch():
    from gnuais_amd import ReceiverNode
    N = 6
    x = seed9(N)
    b, _ = twins(N, max_len=8192)
    nd = ReceiverNode(N, devices=[0, 0], max_len=8192)
    nd.long_frames(True)
    for a in range(0, x.shape[0], 8192):
        b.run(dev(x[a:a + 8192]))
        nd.run_host(x[a:a + 8192])
    nd.sync()
    want = b.drain_long_frames()
    got = nd.drain_long_frames()
    assert len(want) >= 5 * N and got.tobytes() == want.tobytes()
    assert sorted(set(got["channel"].tolist())) == list(range(N))
    key = got["channel"].astype(np.int64) << 40 | ((got["flags"].astype(np.int64) >> 1) << 32) | got["end_bit"]
    assert np.all(np.diff(key) > 0)
    assert np.array_equal(nd.long_counters()[0], b.long_counters()[0])
    nd.close()


def test_decode_file_long_prints_the_long_sentences_behind_each_calls_others(tmp_path):
    """scripts/decode_file.py --long on a written three-channel capture: per call the chain's sentences, then the long
    frames' (the restated reference functions), one sequence digit per channel for both; with --times each long sentence
    behind the TAG block of its own t"""
    import frame_time_ref as ftr
    from gnuais_amd import nmea_tagged_from_frames
    from gnuais_amd.receiver import nmea_from_frames
    x = seed9()
    path = str(tmp_path / "capture.s16")
    x.tofile(path)
    call, start = 5000, 1_700_000_000
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), path, "--raw", "3",
                                     "--call", str(call), *a], check=True, capture_output=True, timeout=300)
    got, tagged, plain = run("--long"), run("--long", "--times", "--start", str(start)), run()
    want = {False: b"", True: b""}
    for times in (False, True):
        short, long_, seq = ftr.FrameTimeRef(3), SampleRef(3), np.zeros(3, dtype=np.uint8)
        done = [0, 0, 0]
        mul, off = ftr.time_map("audio")
        for lo in range(0, x.shape[0], call):
            short.run(x[lo:lo + call])
            long_.run(x[lo:lo + call])
            fr, t = short.drain()
            want[times] += nmea_tagged_from_frames(fr, t, seq, mul, off, 48000, start) if times else nmea_from_frames(fr, seq)
            for c in range(3):
                new = long_.ds[c].long_frames()[done[c]:]
                done[c] += len(new)
                for f in new:
                    text, digit = lr.ref_sentences(f["payload"], f["n"], int(seq[c]))
                    seq[c] = digit
                    if times:
                        body = b"c:%d" % (start + (long_.t(c, f) * mul + off) // 48000)
                        chk = 0
                        for ch in body:
                            chk ^= ch
                        tag = b"\\" + body + b"*%02X" % chk + b"\\"
                        text = b"".join(tag + line + b"\r\n" for line in text.split(b"\r\n")[:-1])
                    want[times] += text
    assert got.stdout == want[False] and tagged.stdout == want[True]
    # (the payloads are random: only those whose first six bits are a type 1 .. 24 give sentences)
    assert got.stdout.count(b"!AIVDM,3,") >= 3 and got.stdout.count(b"!AIVDM") > plain.stdout.count(b"!AIVDM") >= 3
    assert b"15 long frames" in got.stderr
