"""Repair of long frames on the device (gnuais_batch_long_repair: hdlc_long.hip in its form that keeps the raw bits, and
hdlc_long_repair.hip behind it).  Every comparison is against the bit-by-bit restatement tests/long_repair_ref.py; twin
batches get the same calls with the repair off (the records that are not repaired must be theirs) and with everything off
(the chain must not notice)."""
import json
import os

import numpy as np
import pytest

import long_ref as lr
import long_repair_ref as lrr
import repair_ref as rr
from gnuais_amd import synth
from test_iq_gpu import dev
from test_long_gpu import SampleRef, chain_state, fsm_rows, got_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIGMA, SEEDS = 5000.0, (7, 13, 1)       # make_stream with long_ref.long_payloads(): the restatement alone repairs 4, 4, 3
TAIL = np.zeros(3, dtype=np.uint8)


def triplet(n_ch, chain_repair=False, **kw):
    """(long frames and their repair on, long frames only, everything off)"""
    from gnuais_amd import ReceiverBatch
    on, plain, off = (ReceiverBatch(n_ch, **kw) for _ in range(3))
    assert on.info("long_repair") == 0
    on.long_frames(True)
    on.long_repair(True)
    plain.long_frames(True)
    assert on.info("long_repair") == 1 and on.info("long_cand_cap") == on.info("long_frame_cap") and plain.info("long_repair") == 0
    if chain_repair:
        for b in (on, plain, off):
            b.repair(True)
    return on, plain, off


def counters3(b):
    d, f = b.long_counters()
    return np.stack([d, f, b.long_repaired()], axis=1)


def check(b, plain, ds, times=None):
    """one drain and the three counters against the restatement, the unrepaired records against the twin; -> records"""
    got = b.drain_long_frames()
    want, want_counters = lrr.records_of(ds, times)
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    assert np.array_equal(counters3(b), want_counters)
    assert got[(got["flags"] & rr.FRAME_REPAIRED) == 0].tobytes() == plain.drain_long_frames().tobytes()
    assert np.array_equal(counters3(plain)[:, :2], want_counters[:, :2]) and not plain.long_repaired().any()
    return got


def feed_all(batches, ds, part):
    for b in batches:
        b.decode_bits(part)
    for d, p in zip(ds, part):
        d.feed(p)


def test_seventy_channels_two_calls_cut_anywhere():
    """two waves, the second ragged; long bursts with a symbol error, a flipped bit, two symbol errors or nothing"""
    N = 70
    rng = np.random.default_rng(51)
    streams = [lrr.damaged_channel_bits(rng, c) for c in range(N)]
    cuts = [int(rng.integers(1, s.size)) for s in streams]
    b, plain, off = triplet(N, max_len=8192)
    ds = [lrr.RawLongDeframer() for _ in range(N)]
    for part in ([s[:k] for s, k in zip(streams, cuts)], [s[k:] for s, k in zip(streams, cuts)]):
        feed_all((b, plain, off), ds, part)
        assert got_rows(b) == fsm_rows(ds) == got_rows(plain)
    got = check(b, plain, ds)
    rep = got[(got["flags"] & rr.FRAME_REPAIRED) != 0]
    assert len(rep) > 20 and len(got) - len(rep) > 20 and (got["t"] == -1).all()
    assert {int(n) for n in rep["nbits"]} >= {432, 480, 640, 800, 1008} and 1016 not in got["nbits"]
    c3 = counters3(b)
    assert c3[:, 1].sum() > c3[:, 2].sum() + 20         # flipped bits and two symbol errors stay lost
    assert chain_state(b) == chain_state(off) and b.pending_long_frames() == 0


def test_one_damaged_burst_cut_at_every_bit():
    """a 126-byte burst with a symbol error; channel c gets its first c bits in call 1 and the rest in call 2: D''s open
    record, raw, carries across the calls wherever the cut lies"""
    rng = np.random.default_rng(52)
    s = lr.burst(rng.integers(0, 256, 126, dtype=np.uint8)).copy()
    s[611:613] ^= 1
    s = np.concatenate([s, TAIL])
    N = s.size + 1
    d = lrr.RawLongDeframer()
    before = []
    d.feed(s, states=before)
    before.append(d.fields())
    assert d.long_counters() == (0, 1)
    b, plain, off = triplet(N, max_len=8192)
    fed = np.zeros(N, dtype=np.int64)
    for call in ([s[:c] for c in range(N)], [s[c:] for c in range(N)]):
        for q in (b, plain, off):
            q.decode_bits(call)
        fed += [len(x) for x in call]
        assert got_rows(b) == [before[i] for i in fed]
    one, c3 = lrr.records_of([d])                           # the restatement's repair once: every channel has these bits
    assert len(one) == 1 and c3.tolist() == [[0, 1, 1]]
    want = np.repeat(one, N)
    want["channel"] = np.arange(N)
    got = b.drain_long_frames()
    assert got.tobytes() == want.tobytes() and (got["flags"] == 0x41).all() and (got["nbits"] == 1008).all()
    assert np.array_equal(counters3(b), np.tile(c3, (N, 1)))
    assert len(plain.drain_long_frames()) == 0 and np.array_equal(counters3(plain), np.tile([0, 1, 0], (N, 1)))
    assert chain_state(b) == chain_state(off)


def crafted(nbytes, seed):
    """a payload with five 1s and their stuffed zero at a known place, and 1111 0 1 at another: (payload, its burst, the
    burst's index of the fifth 1, of the 0 behind the four 1s)"""
    payload = bytearray(np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8))
    payload[5:8] = bytes([0x00, 0x1F, 0x00])
    payload[10:13] = bytes([0x00, 0x2F, 0x00])
    burst = lr.burst(np.frombuffer(bytes(payload), dtype=np.uint8))
    body = burst[32:]
    a = next(i for i in range(40, 80) if body[i - 5:i + 2].tolist() == [0, 1, 1, 1, 1, 1, 0] and not body[i + 2]) + 32
    k = next(i for i in range(a - 32 + 8, a - 32 + 60) if body[i - 5:i + 2].tolist() == [0, 1, 1, 1, 1, 0, 1]) + 32
    return bytes(payload), burst, a, k


def with_pair(burst, p):
    out = burst.copy()
    out[p:p + 2] ^= 1
    return np.concatenate([out, TAIL])


def test_limits_ambiguous_fixtures_and_both_repairs_side_by_side():
    """both repairs on: each damaged frame is delivered exactly once, by the repair that owns it, or stays lost"""
    from oracle_lib import FRAME_DTYPE
    rng = np.random.default_rng(53)
    while True:
        p_limit = rng.integers(0, 256, 126, dtype=np.uint8) & 0x77          # 1030 stored bits and not one stuffed zero
        if lrr.candidate_raw(p_limit).size == 1030:
            break
    with open(os.path.join(ROOT, "tests", "golden", "long_repair_ambiguous.json")) as f:
        fixtures = json.load(f)
    p53, b53, a53, _ = crafted(53, 60)
    p54, b54, _, k54 = crafted(54, 61)
    streams = {
        "at the limit": with_pair(lr.burst(p_limit), 600),
        "all ones": with_pair(lr.burst(np.full(126, 0xFF, dtype=np.uint8)), 900),
        "127 bytes": with_pair(lr.burst(rng.integers(0, 256, 127, dtype=np.uint8)), 300),
        "424 bits, a stuffed zero destroyed": with_pair(b53, a53),
        "432 bits, a stuffed zero made": with_pair(b54, k54),
        "undamaged": np.concatenate([lr.burst(rng.integers(0, 256, 80, dtype=np.uint8)), TAIL]),
    }
    for i, fx in enumerate(fixtures):
        streams[f"ambiguous {i}"] = with_pair(lr.burst(np.frombuffer(bytes.fromhex(fx["payload"]), dtype=np.uint8)), 32 + fx["p1"])
    names, bits = list(streams), list(streams.values())
    N = len(bits)
    b, plain, off = triplet(N, chain_repair=True, max_len=8192)
    ds = [lrr.RawLongDeframer() for _ in range(N)]
    feed_all((b, plain, off), ds, bits)
    got = check(b, plain, ds)
    by = {names[int(r["channel"])]: r for r in got}
    # (the all-ones frame is the restatement's to decide: in runs of five 1s and a 0 several pairs undo the same error)
    assert sorted(set(by) - {"all ones"}) == ["432 bits, a stuffed zero made", "at the limit", "undamaged"]
    assert int(counters3(b)[names.index("all ones"), 1]) == 1
    assert by["432 bits, a stuffed zero made"]["flags"] == 0x41 and bytes(by["432 bits, a stuffed zero made"]["payload"][:54]) == p54
    assert by["at the limit"]["nbits"] == 1008 and by["undamaged"]["flags"] == 1
    c3 = counters3(b)
    assert [int(v) for v in c3[names.index("127 bytes")]] == [0, 0, 0]     # given up at 1031 stored bits: no candidate at all
    assert all([int(v) for v in c3[names.index(n)]] == [0, 1, 0] for n in names if n.startswith("ambiguous"))
    # the chain's own repair on the same bits: the 424-bit frame is its, and nothing else
    want_short, want_rep, _ = rr.decode_streams(bits)
    short = b.drain_frames()
    ws = np.zeros(len(want_short), dtype=FRAME_DTYPE)
    for i, r in enumerate(want_short):
        ws[i] = r
    assert short.tobytes() == ws.tobytes() and len(short) == 1 and short["flags"][0] == 0x41
    assert names[int(short["channel"][0])] == "424 bits, a stuffed zero destroyed" and bytes(short["payload"][0][:53]) == p53
    assert np.array_equal(b.repaired(), want_rep) and short.tobytes() == off.drain_frames().tobytes()
    assert np.array_equal(b.counters(), off.counters()) and b.fsm_state().tobytes() == off.fsm_state().tobytes()


def noisy(n_ch=len(SEEDS)):
    return np.stack([synth.make_stream(6 * 8 * 1280, seed=SEEDS[c % len(SEEDS)], sigma=SIGMA, payloads=lr.long_payloads())[0]
                     for c in range(n_ch)], axis=1)


def test_a_noisy_stream_through_run_with_the_times_of_repaired_records():
    """(at the sigma of tests/test_long_cpu.py, 3000, no long frame of fifty seeds fails its CRC; at 5000 most do)"""
    x = noisy()
    N = x.shape[1]
    b, plain, off = triplet(N, max_len=8192)
    ref = SampleRef(N)
    ref.ds = [lrr.RawLongDeframer() for _ in range(N)]
    for a in range(0, x.shape[0], 8192):
        for q in (b, plain, off):
            q.run(dev(x[a:a + 8192]))
        ref.run(x[a:a + 8192])
        assert got_rows(b) == fsm_rows(ref.ds)
    got = check(b, plain, ref.ds, ref.t)
    rep = got[(got["flags"] & rr.FRAME_REPAIRED) != 0]
    assert [int(v) for v in b.long_repaired()] == [4, 4, 3] and len(rep) == 11
    assert rep["t"].min() > 0 and rep["t"].max() < x.shape[0] and len(got) > len(rep)
    assert chain_state(b) == chain_state(off)


def test_decode_file_long_repair_implies_long_and_counts_the_repairs(tmp_path):
    """scripts/decode_file.py --long-repair on the same three noisy channels, written as a capture: the sentences of
    --long and more, and the summary counts the restatement's 2 received and 11 repaired long frames"""
    import subprocess
    import sys
    path = str(tmp_path / "capture.s16")
    noisy().tofile(path)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), path, "--raw", "3",
                                     "--call", "8192", *a], check=True, capture_output=True, timeout=300)
    plain, rep = run("--long"), run("--long-repair")
    assert b"2 long frames (more than two slots)\n" in plain.stderr and b"repaired" not in plain.stderr
    assert b"13 long frames (more than two slots), 11 of them repaired\n" in rep.stderr
    assert rep.stdout.count(b"!AIVDM") > plain.stdout.count(b"!AIVDM")      # (the sequence digits of the later ones move)


def test_switch_order_resets_streaming_and_an_overflow_made_by_repairs():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_OVERFLOW, E_STATE, GnuaisError
    N = 4
    b = ReceiverBatch(N, max_len=8192)
    with pytest.raises(GnuaisError) as e:
        b.long_repair(True)                                 # not without long frames
    assert e.value.code == E_STATE and b.info("long_repair") == 0
    b.long_frames(True)
    b.long_repair(True)
    b.long_frames(False)                                    # off together with long frames
    assert b.info("long_repair") == 0 and b.info("long_frames") == 0
    b.long_frames(True)
    assert b.info("long_repair") == 0
    b.long_repair(True)
    rng = np.random.default_rng(54)
    one = with_pair(lr.burst(rng.integers(0, 256, 54, dtype=np.uint8)), 200)
    d = lrr.RawLongDeframer()
    d.feed(one)
    assert lrr.records_of([d])[1].tolist() == [[0, 1, 1]]
    # a frame damaged in one call and closed after the switch went on: `open` is raw in either form
    b.long_repair(False)
    b.decode_bits([one[:300]] * N)
    b.long_repair(True)
    b.decode_bits([one[300:]] * N)
    assert len(b.drain_long_frames()) == N and np.array_equal(counters3(b), np.tile([0, 1, 1], (N, 1)))
    b.protodec_reset()                                      # keeps the counters
    assert np.array_equal(counters3(b), np.tile([0, 1, 1], (N, 1)))
    b.decode_bits([one] * N)
    assert np.array_equal(counters3(b), np.tile([0, 2, 2], (N, 1)))
    b.reset()                                               # zeroes them, and the ring
    assert not counters3(b).any() and b.pending_long_frames() == 0 and b.info("long_repair") == 1
    # the long ring made to overflow by repairs alone: GNUAIS_E_OVERFLOW, the oldest kept, the counters exact
    cap = int(b.info("long_frame_cap"))
    per = cap // N + 2
    for _ in range(per):
        b.decode_bits([one] * N)
    with pytest.raises(GnuaisError) as e:
        b.drain_long_frames()
    assert e.value.code == E_OVERFLOW and len(e.value.frames) == cap and (e.value.frames["flags"] & 0x40).all()
    assert np.array_equal(counters3(b), np.tile([0, per, per], (N, 1))) and b.pending_long_frames() == 0
    # streaming, both ways
    for call in (b.stream_nmea, lambda: b.set_option("streaming", 1)):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    b.long_frames(False)
    b.stream_nmea()
    for call in (lambda: b.long_frames(True), lambda: b.long_repair(True)):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    b.set_option("streaming", 0)


def test_a_node_of_two_shards_equals_one_batch():
    from gnuais_amd import ReceiverBatch, ReceiverNode
    N = 6
    x = noisy(N)
    b = ReceiverBatch(N, max_len=8192)
    nd = ReceiverNode(N, devices=[0, 0], max_len=8192)
    for q in (b, nd):
        q.long_frames(True)
        q.long_repair(True)
    for a in range(0, x.shape[0], 8192):
        b.run(dev(x[a:a + 8192]))
        nd.run_host(x[a:a + 8192])
    nd.sync()
    want = b.drain_long_frames()
    got = nd.drain_long_frames()
    assert got.tobytes() == want.tobytes() and int((got["flags"] & 0x40 != 0).sum()) == 22
    assert np.array_equal(nd.long_repaired(), b.long_repaired()) and nd.long_repaired().tolist() == [4, 4, 3, 4, 4, 3]
    assert np.array_equal(nd.long_counters()[1], b.long_counters()[1])
    nd.long_frames(False)
    nd.close()
