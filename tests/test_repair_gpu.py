"""Single-symbol repair on the device (gnuais_batch_repair, hdlc_repair.hip) against the brute-force restatement
(tests/repair_ref.py): crafted bit streams through decode_bits over batch sizes and both deframer forms, noisy streams
through run in ragged calls, the feature off, and the feature beside the receive times, the streamed delivery, the
resets, a ring that overflows and a node."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import frame_time_ref as ftr
import repair_ref as rr
from gnuais_amd import synth
from oracle_lib import FRAME_DTYPE, Oracle
from test_iq_gpu import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GAP = [0] * 40
RAGGED = [1, 777, 2048, 2049]


def records(recs):
    out = np.zeros(len(recs), dtype=FRAME_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out


def counters3(b):
    cnt = b.counters()
    return np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1)


def flipped_frame(payload, p):
    """the on-air bits of a frame whose raw bits p and p + 1 (counted as the deframer records them) are inverted"""
    bits = synth.hdlc_frame_bits(payload).copy()
    bits[32 + p] ^= 1
    bits[32 + p + 1] ^= 1
    return bits.tolist()


def stuffing_positions(payload):
    """raw indices: a = the fifth 1 in front of a stuffed zero, b = the 0 of a 1111 0 1 (tests/test_repair_cpu.py)"""
    from test_repair_cpu import stuffed_with_map
    raw, where = stuffed_with_map(payload)
    return raw, where[6 * 8 + 4], where[11 * 8 + 4]


def crafted_payload(rng, nbytes):
    payload = bytearray(rng.integers(0, 256, nbytes, dtype=np.uint8))
    payload[5:8] = bytes([0x00, 0x1F, 0x00])
    payload[10:13] = bytes([0x00, 0x2F, 0x00])
    payload[0], payload[3], payload[4], payload[8] = 0xAA, 0x55, 0x55, 0x55     # no run of 1s for a pair at 0, 30 .. 32, 62 .. 64 to lengthen to six
    return bytes(payload)


def crafted_channel(c):
    """channel c's stream: a frame with one pair inverted, then an untouched one; -> (bits, payload A, payload B, p)"""
    rng = np.random.default_rng([77, c])
    nbytes = (21, 53)[c % 2]
    pa, pb = crafted_payload(rng, nbytes), bytes(rng.integers(0, 256, (53, 21)[c % 2], dtype=np.uint8))
    raw, a, b = stuffing_positions(pa)
    ps = [0, 30, 31, 32, a, b, 62, 63, 64, raw.size - 9]
    p = ps[(c // 2) % len(ps)]
    bits = GAP + flipped_frame(pa, p) + GAP + synth.hdlc_frame_bits(pb).tolist() + GAP
    return np.array(bits, dtype=np.uint8), pa, pb, p


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n_ch", [1, 3, 33, 65])
def test_crafted_frames_through_decode_bits(n_ch, variant):
    from gnuais_amd import ReceiverBatch
    made = [crafted_channel(c if n_ch > 3 else c + 2 * n_ch) for c in range(n_ch)]
    streams = [m[0] for m in made]
    want, want_rep, want_cnt = rr.decode_streams(streams)
    want = records(want)
    # what the restatement says is what the issue states: one repaired frame, one untouched, per channel
    assert np.array_equal(want_rep, np.ones(n_ch)) and np.array_equal(want_cnt, np.tile([1, 1, 0], (n_ch, 1)))
    for c, (_, pa, pb, _) in enumerate(made):
        mine = want[want["channel"] == c]
        assert [bytes(f["payload"][: f["nbits"] // 8]) for f in mine] == [pa, pb]
        assert [int(f["flags"]) & 0x40 for f in mine] == [0x40, 0]
    o = Oracle(n_ch)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    # off: no frame from the damaged one, lostframes 1
    b = ReceiverBatch(n_ch)
    b.set_option("hdlc_variant", variant)
    assert b.info("repair") == 0
    b.decode_bits(streams)
    assert b.drain_frames().tobytes() == o.frames().tobytes()
    assert np.array_equal(counters3(b), o.counters()) and np.array_equal(counters3(b), want_cnt)
    assert not b.repaired().any()
    # on
    b.reset()
    b.repair(True)
    assert b.info("repair") == 1
    b.decode_bits(streams)
    got = b.drain_frames()
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    assert np.array_equal(counters3(b), want_cnt) and np.array_equal(b.repaired(), want_rep)


def ambiguous_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "repair_ambiguous.json")) as f:
        return json.load(f)[0]


def test_three_failed_frames_per_channel_an_ambiguous_one_and_two_symbol_errors():
    from gnuais_amd import ReceiverBatch
    n_ch = 33
    fx = ambiguous_fixture()
    streams = []
    for c in range(n_ch):
        rng = np.random.default_rng([78, c])
        bits = list(GAP)
        for j in range(3):
            payload = bytes(rng.integers(0, 256, (21, 53)[(c + j) % 2], dtype=np.uint8))
            raw = rr.candidate_raw(payload)
            while True:             # a pair that makes six 1s closes the frame early: not this test's case
                p = int(rng.integers(0, raw.size - 8))
                r = raw.copy()
                r[p:p + 2] ^= 1
                if "111111" not in "".join(map(str, r)):
                    break
            bits += flipped_frame(payload, p) + GAP
        if c % 3 == 0:          # two different trials repair it: stays lost
            bits += flipped_frame(bytes.fromhex(fx["payload"]), fx["p1"]) + GAP
        if c % 3 == 1:          # two symbol errors: stays lost
            payload = bytes(rng.integers(0, 256, 21, dtype=np.uint8))
            f = np.array(flipped_frame(payload, 20))
            f[32 + 90] ^= 1
            f[32 + 91] ^= 1
            bits += f.tolist() + GAP
        streams.append(np.array(bits, dtype=np.uint8))
    want, want_rep, want_cnt = rr.decode_streams(streams)
    assert want_rep.sum() >= 2 * n_ch and want_cnt[:, 0].sum() == 0
    assert np.array_equal(want_cnt[:, 1], [4 if c % 3 < 2 else 3 for c in range(n_ch)])
    assert np.all(want_rep <= 3)                    # neither the ambiguous frame nor the doubly damaged one comes back
    b = ReceiverBatch(n_ch)
    b.repair(True)
    b.decode_bits(streams)
    assert b.drain_frames().tobytes() == records(want).tobytes()
    assert np.array_equal(counters3(b), want_cnt) and np.array_equal(b.repaired(), want_rep)


N_CH, ROWS = 65, 96000


@pytest.fixture(scope="module")
def noisy():
    """65 channels x 96 000 samples of make_stream at sigma 6000: the input, the oracle's frames and counters, the
    restatement's frames (the oracle's and the repairs), repairs per channel"""
    x = np.stack([synth.make_stream(ROWS, seed=20, channel=c, amplitude=12000.0, sigma=6000.0, occupancy=0.5)[0]
                  for c in range(N_CH)], axis=1)
    o = Oracle(N_CH)
    bits = o.run(x, want_bits=True)["bits"]
    frames, repaired, counters = rr.decode_streams(bits)
    frames = records(frames)
    of = o.frames()
    assert np.array_equal(counters, o.counters())
    assert frames[(frames["flags"] & 0x40) == 0].tobytes() == of.tobytes()      # the union: the oracle's frames ...
    assert int(((frames["flags"] & 0x40) != 0).sum()) == repaired.sum() > N_CH  # ... and the restatement's repairs
    return x, of, o.counters(), frames, repaired


def ragged_calls(b, xd, sync):
    cuts = np.cumsum([0] + RAGGED + [ROWS - sum(RAGGED)])
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e], sync=sync)


def test_noisy_streams_through_run_in_ragged_calls(noisy):
    from gnuais_amd import ReceiverBatch
    x, _, counters, frames, repaired = noisy
    xd = dev(x)
    b = ReceiverBatch(N_CH, max_len=ROWS)
    b.repair(True)
    for sync in (True, False):              # a sync after every call; then the same calls queued
        ragged_calls(b, xd, sync)
        got = b.drain_frames()
        assert got.tobytes() == frames.tobytes(), (sync, len(got), len(frames))
        assert np.array_equal(counters3(b), counters) and np.array_equal(b.repaired(), repaired)
        b.reset()
        assert not b.repaired().any() and b.info("repair") == 1


def test_with_the_feature_off_the_oracle(noisy):
    from gnuais_amd import ReceiverBatch
    x, of, counters, _, _ = noisy
    xd = dev(x)
    never, was = ReceiverBatch(N_CH, max_len=ROWS), ReceiverBatch(N_CH, max_len=ROWS)
    was.repair(True)
    was.repair(False)
    assert was.info("repair") == 0
    for b in (never, was):
        ragged_calls(b, xd, False)
        assert b.drain_frames().tobytes() == of.tobytes()
        assert np.array_equal(counters3(b), counters) and not b.repaired().any()


def test_repaired_frames_get_their_receive_time(noisy):
    from gnuais_amd import ReceiverBatch
    n_ch, calls = 9, [1, 777, 2048, 2049, 15000]
    x = noisy[0][: sum(calls), :n_ch]
    b = ReceiverBatch(n_ch, max_len=max(calls))
    b.repair(True)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch)
    pos = 0
    for n in calls:
        b.run(dev(x[pos:pos + n]), sync=False)
        ref.run(x[pos:pos + n])
        pos += n
    segs = list(ref.segs)
    wf, wt = ref.drain()
    fr, t = b.drain_frames_timed()
    rep = (fr["flags"] & 0x40) != 0
    assert fr[~rep].tobytes() == wf.tobytes() and np.array_equal(t[~rep], wt)
    assert rep.sum() >= 5 and rep.sum() == b.repaired().sum()
    base = np.stack([s[2] for s in segs])
    for i in np.nonzero(rep)[0]:                    # frame_time_ref's rule for the repaired frame's stamp
        c, e, ti = int(fr["channel"][i]), int(ftr.stamp(fr[i:i + 1])[0]), int(t[i])
        k = int(np.searchsorted(base[:, c], e, side="right")) - 1
        row0, l_s, b0, cnt = segs[k]
        assert ti >= 0 and ti == ftr.interp(row0, 0, e - int(b0[c]), l_s, int(cnt[c]))
    order = np.lexsort((ftr.stamp(fr), fr["channel"]))
    assert np.array_equal(order, np.arange(len(fr)))            # repaired frames stand where their stamp puts them


def test_streaming_refusals_and_the_resets(noisy):
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_STATE, GnuaisError
    n_ch, rows = 9, 20000
    x = noisy[0][:rows, :n_ch]
    b = ReceiverBatch(n_ch, max_len=rows)
    b.repair(True)
    for call in (b.stream_nmea, lambda: b.set_option("streaming", 1)):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    b.run(dev(x))
    rep = b.repaired()
    assert rep.sum() >= 5
    b.protodec_reset()
    assert np.array_equal(b.repaired(), rep)        # protodec_reset keeps it, as it keeps the reference's three
    b.reset()
    assert not b.repaired().any() and b.pending_frames() == 0
    b.repair(False)
    b.stream_nmea()                                 # a streaming batch refuses the feature, in both directions
    for on in (True, False):
        with pytest.raises(GnuaisError) as e:
            b.repair(on)
        assert e.value.code == E_STATE
    b.set_option("streaming", 0)
    b.repair(True)
    assert b.info("repair") == 1


def test_a_ring_that_overflows_and_a_node_of_two_shards(noisy):
    from gnuais_amd import ReceiverBatch, ReceiverNode, lib
    x, _, counters, frames, repaired = noisy
    half = ROWS // 2
    # frame_capacity 64: K3's frames and the repairs together overflow it
    b = ReceiverBatch(N_CH, max_len=half, frame_capacity=64)
    b.repair(True)
    b.run(dev(x[:half]))
    out = np.zeros(4096, dtype=FRAME_DTYPE)
    got = C.c_int()
    rc = b._lib.gnuais_batch_drain_frames(b._h, out.ctypes.data, int(out.size), C.byref(got))
    assert rc == lib.E_OVERFLOW and 0 < got.value <= 64
    have = {bytes(f.tobytes()) for f in frames}
    assert all(bytes(f.tobytes()) in have for f in out[: got.value])
    b.run(dev(x[half:]))                            # the counters stay exact
    rc = b._lib.gnuais_batch_drain_frames(b._h, out.ctypes.data, int(out.size), C.byref(got))
    assert rc in (lib.OK, lib.E_OVERFLOW)
    assert np.array_equal(counters3(b), counters) and np.array_equal(b.repaired(), repaired)
    nd = ReceiverNode(N_CH, devices=[0, 0], max_len=half)
    nd.repair(True)
    nd.run_host(x[:half])
    nd.run_host(x[half:])
    nd.sync()
    assert nd.drain_frames().tobytes() == frames.tobytes()
    assert np.array_equal(nd.repaired(), repaired)
    nd.close()
