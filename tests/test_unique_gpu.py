"""One record per transmission on the device (gnuais_batch_unique, frame_unique.hip).  The expected value is always
tests/unique_ref.py applied to what drain_frames_timed() of a TWIN batch gives for the same calls -- a path that exists
and is tested by itself -- so the new drain is never compared with itself: receivers that hear the same transmissions,
drained once and after every ragged call; a cluster wider than a workgroup; a chain; late copies across a drain; an
intact copy before a repaired one; forced hash collisions; untimed frames and the small sizes; the switch and its
states; I/Q and wideband input; a node; one larger shape."""
import ctypes as C

import numpy as np
import pytest

import unique_ref as ur
from gnuais_amd import synth
from gnuais_amd.lib import E_ARG, E_STATE, FRAME_DTYPE, GnuaisError
from test_iq_gpu import dev
from test_repair_gpu import crafted_payload, flipped_frame

pytestmark = pytest.mark.gpu
GAP = [0] * 40


def pair(n_ch, W, max_len=ur.TOTAL, repair=False, hash_bits=64):
    """the batch under test and its twin, which only times its frames"""
    from gnuais_amd import ReceiverBatch
    b, t = ReceiverBatch(n_ch, max_len=max_len), ReceiverBatch(n_ch, max_len=max_len)
    for x in (b, t):
        if repair:
            x.repair(True)
        x.frame_times(True)
    assert b.info("unique") == 0
    b.unique(W)
    assert b.info("unique") == W
    if hash_bits != 64:
        b.set_option("unique_hash_bits", hash_bits)
    return b, t


class Check:
    """drain by drain: the unique drain of `b` against the restatement over the twin's timed drain"""

    def __init__(self, b, t, W):
        self.b, self.t, self.ref = b, t, ur.UniqueRef(W)
        self.twin_frames = self.copies = self.records = 0

    def drain(self):
        got = self.b.drain_frames_unique()
        fr, tm = self.t.drain_frames_timed()
        rows = int(self.t.info("rows"))
        assert rows == int(self.b.info("rows"))
        want = self.ref.push(fr, tm, rows)
        assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]), len(fr))
        assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32, (got[2], want[2])
        assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int64
        assert got[0].tobytes() == want[0].tobytes()
        assert self.b.unique_late() == self.ref.late == int(self.b.info("unique_late"))
        self.twin_frames += len(fr)
        self.copies += int(got[2].sum())
        self.records += len(got[0])
        assert self.copies + self.b.unique_late() == self.twin_frames
        assert self.b.pending_frames() == 0
        return got


def run_calls(b, t, x, cuts, each=None):
    xd = dev(x)
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        if each:
            each()


@pytest.fixture(scope="module")
def seventy():
    return ur.receivers(10, ur.DELAYS7)


@pytest.mark.parametrize("per_call", [False, True])
def test_six_receivers_drained_once_and_after_every_ragged_call(per_call):
    x = ur.receivers(1, ur.DELAYS6)
    b, t = pair(6, 128)
    ck = Check(b, t, 128)
    run_calls(b, t, x, ur.ragged_cuts(), ck.drain if per_call else None)
    got = ck.drain()
    assert ck.twin_frames == 48 and ck.records == 8
    if not per_call:
        assert got[2].tolist() == [6] * 8 and b.unique_late() == 0


@pytest.mark.parametrize("hash_bits", [64, 1, 3])
@pytest.mark.parametrize("per_call", [False, True])
def test_seventy_receivers_and_forced_hash_collisions(seventy, per_call, hash_bits):
    """10 groups x 7 delays; with the hash cut to 1 and 3 bits different keys share a hash in every drain and the exact
    path gives the same records"""
    b, t = pair(70, 128, hash_bits=hash_bits)
    ck = Check(b, t, 128)
    run_calls(b, t, seventy, ur.ragged_cuts(), ck.drain if per_call else None)
    got = ck.drain()
    assert ck.twin_frames > 500 and 80 <= ck.records <= 90
    if not per_call:
        assert got[2].max() == 7 and np.count_nonzero(got[2] == 7) > 60


def test_a_cluster_wider_than_a_workgroup():
    """300 channels carry one payload stream, delays c % 41"""
    one = ur.receivers(1, [0])[:, 0]
    rng = np.random.default_rng(5)
    x = np.stack([np.roll(one, c % 41) for c in range(300)], axis=1).astype(np.int32)
    x = np.clip(x + rng.normal(0.0, 300.0, x.shape).round().astype(np.int32), -32768, 32767).astype(np.int16)
    b, t = pair(300, 128)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, ur.TOTAL])
    got = ck.drain()
    assert ck.records == 8 and np.count_nonzero(got[2] > 256) >= 6 and got[2].max() == 300


def slots_stream(total, slot_payloads, seed=21, channel=0, sigma=300.0):
    """a channel with the given {slot: payload}"""
    return synth.make_stream(total, seed=seed, channel=channel, sigma=sigma,
                             payloads=lambda rng, slot: slot_payloads.get(slot))[0]


@pytest.mark.parametrize("W,clusters", [(1300, 1), (1200, 8)])
def test_a_chain_of_copies_one_slot_apart(W, clusters):
    """one payload in consecutive slots on alternating channels: the copies lie 1280 rows apart"""
    p = synth.random_position_report(np.random.default_rng(1))
    x = np.stack([slots_stream(ur.TOTAL, {s: p for s in range(8) if s % 2 == c}, channel=c) for c in range(2)], axis=1)
    b, t = pair(2, W)
    ck = Check(b, t, W)
    run_calls(b, t, x, [0, ur.TOTAL])
    got = ck.drain()
    assert ck.twin_frames == 8 and got[2].tolist() == [8 // clusters] * clusters


def late_input(delays):
    """slot 1 on every channel (delayed), and the same payload once more in slot 5 of channel 0"""
    p = synth.random_position_report(np.random.default_rng(2))
    cols = [np.roll(slots_stream(ur.TOTAL, {1: p, 5: p} if c == 0 else {1: p}, channel=c), d)
            for c, d in enumerate(delays)]
    return np.stack(cols, axis=1)


def test_late_copies_across_a_drain():
    """delays 0 and 600, W = 700, the cut between the ends of the two copies: the second drain delivers nothing for the
    transmission and counts one late copy; W rows later the tail is empty and the same payload is a transmission again"""
    x = late_input([0, 600])
    b, t = pair(2, 700)
    ck = Check(b, t, 700)
    xd = dev(x)
    for (a, e), (n_rec, late) in zip([(0, 2800), (2800, 5000), (5000, ur.TOTAL)], [(1, 0), (0, 1), (1, 1)]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        got = ck.drain()
        assert len(got[0]) == n_rec and b.unique_late() == late, (a, e, len(got[0]), b.unique_late())
        assert got[2].tolist() == [1] * n_rec
    assert ck.twin_frames == 3


def test_reset_clears_and_protodec_reset_keeps_the_tail_and_the_count():
    x = late_input([0, 600, 2000])
    xd = dev(x)
    b, t = pair(3, 2000)
    ck = Check(b, t, 2000)
    for (a, e), (n_rec, late) in zip([(0, 2800), (2800, 3200), (3200, 5200)], [(1, 0), (0, 1), (0, 2)]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        got = ck.drain()
        assert len(got[0]) == n_rec and b.unique_late() == late
        if e == 3200:                   # between the second copy's end and the third one's start
            b.protodec_reset()
            t.protodec_reset()
            assert b.unique_late() == 1
    # reset: rows start again at 0; a kept tail entry (t_last about 4400) would swallow the first copy as a late one
    b.reset()
    t.reset()
    ck = Check(b, t, 2000)
    assert b.unique_late() == 0 and b.info("unique") == 2000
    b.run(xd[:5200])
    t.run(xd[:5200])
    got = ck.drain()
    assert got[2].tolist() == [3] and b.unique_late() == 0
    # switching the feature clears both as well
    b.run(xd[5200:5300])
    t.run(xd[5200:5300])
    b.unique(0)
    assert b.info("unique") == 0 and b.unique_late() == 0
    b.unique(2000)
    assert b.unique_late() == 0


def square(bits, start, total, amplitude=12000):
    """an unshaped NRZI square wave of the on-air bits, 5 rows a bit, from row `start`; silence around it"""
    x = np.zeros(total, dtype=np.int16)
    lev = np.repeat(synth.nrzi_levels(np.asarray(bits, dtype=np.uint8)), 5) * amplitude
    x[start:start + lev.size] = lev.astype(np.int16)
    return x


@pytest.mark.parametrize("both_damaged", [False, True])
def test_the_intact_copy_is_handed_on_before_a_repaired_one(both_damaged):
    payload = crafted_payload(np.random.default_rng(4), 21)
    bad, good = flipped_frame(payload, 30), synth.hdlc_frame_bits(payload).tolist()
    x = np.stack([square(bad, 100, 2048), square(bad if both_damaged else good, 120, 2048)], axis=1)
    b, t = pair(2, 128, max_len=2048, repair=True)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, 2048])
    f, tm, c = ck.drain()
    assert ck.twin_frames == 2 and c.tolist() == [2]
    assert bytes(f[0]["payload"][:21]) == payload
    if both_damaged:
        assert int(f[0]["channel"]) == 0 and int(f[0]["flags"]) & ur.REPAIRED
    else:
        assert int(f[0]["channel"]) == 1 and not int(f[0]["flags"]) & ur.REPAIRED


def three_payloads(n_ch, total=2048):
    """n_ch noise-free receivers, each hears one frame in slot 0: payload c % 3, delay c % 41 -- exactly n_ch frames"""
    rng = np.random.default_rng(6)
    pays = [synth.random_position_report(rng) for _ in range(3)]
    base = [slots_stream(total, {0: pays[k]}, seed=6, channel=k, sigma=0.0) for k in range(3)]
    return np.stack([np.roll(base[c % 3], c % 41) for c in range(n_ch)], axis=1)


@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 255, 256, 257])
def test_drains_of_a_chosen_number_of_frames(n_ch):
    b, t = pair(n_ch, 128, max_len=2048)
    ck = Check(b, t, 128)
    got = ck.drain()                            # a drain of 0 frames
    assert len(got[0]) == 0 and got[0].dtype == FRAME_DTYPE
    run_calls(b, t, three_payloads(n_ch), [0, 2048])
    got = ck.drain()
    assert ck.twin_frames == n_ch and ck.records == min(n_ch, 3) and int(got[2].sum()) == n_ch


def test_untimed_frames_come_first_each_by_itself():
    n_ch = 5
    rng = np.random.default_rng(8)
    pay = [synth.random_position_report(rng) for _ in range(2)]
    streams = [np.array(GAP + synth.hdlc_frame_bits(pay[c % 2]).tolist() + GAP + synth.hdlc_frame_bits(pay[0]).tolist() + GAP,
                        dtype=np.uint8) for c in range(n_ch)]
    b, t = pair(n_ch, 128, max_len=2048)
    ck = Check(b, t, 128)
    b.decode_bits(streams)
    t.decode_bits(streams)
    f, tm, c = ck.drain()                       # a drain that holds only t = -1 frames
    assert len(f) == 2 * n_ch and np.all(tm == -1) and np.all(c == 1)
    b.decode_bits(streams)
    t.decode_bits(streams)
    x = three_payloads(n_ch)
    run_calls(b, t, x, [0, 2048])
    f, tm, c = ck.drain()                       # mixed: the untimed ones first, in the plain drain's order
    assert np.all(tm[: 2 * n_ch] == -1) and np.all(tm[2 * n_ch:] >= 0) and len(f) == 2 * n_ch + 3
    assert np.all(c[: 2 * n_ch] == 1) and sorted(c[2 * n_ch:].tolist()) == [1, 2, 2]
    assert f["channel"][: 2 * n_ch].tolist() == sorted(f["channel"][: 2 * n_ch].tolist())


def test_the_switch_and_its_states():
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle

    def state_error(fn, *a):
        with pytest.raises(GnuaisError) as e:
            fn(*a)
        assert e.value.code == E_STATE, e.value

    x = ur.receivers(1, ur.DELAYS6)
    b = ReceiverBatch(6, max_len=ur.TOTAL)
    assert b.info("unique") == 0 and b.info("unique_late") == 0      # off by default
    state_error(b.unique, 128)                  # frame times are off
    state_error(b.drain_frames_unique)          # the feature is off
    b.frame_times(True)
    state_error(b.drain_frames_unique)
    b.unique(128)
    state_error(b.frame_times, False)           # the merge needs the times
    state_error(b.stream_nmea)                  # the three ways into streaming
    state_error(b.set_option, "streaming", 1)
    state_error(b.autotune_delivery, dev(x[:2048]))
    with pytest.raises(GnuaisError):
        b.set_option("unique_hash_bits", 0)
    with pytest.raises(GnuaisError):
        b.set_option("unique_hash_bits", 65)
    # every other drain works as before while the feature is on: the oracle's bytes
    o = Oracle(6)
    o.run(x)
    b.run(dev(x))
    assert b.drain_frames().tobytes() == o.frames().tobytes()
    b.reset()
    b.run(dev(x))
    fr, tm = b.drain_frames_timed()
    assert fr.tobytes() == o.frames().tobytes() and tm.min() >= 0
    # too little room: GNUAIS_E_ARG and nothing consumed
    b.reset()
    b.run(dev(x))
    n = b.pending_frames()
    assert n == 48
    out, tms, cps = np.zeros(n, dtype=FRAME_DTYPE), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    got = C.c_int(-1)
    rc = b._lib.gnuais_batch_drain_frames_unique(b._h, out.ctypes.data, tms.ctypes.data, cps.ctypes.data, n - 1, C.byref(got))
    assert rc == E_ARG and got.value == 0 and b.pending_frames() == n
    f, tm2, c = b.drain_frames_unique()
    assert c.tolist() == [6] * 8
    b.unique(0)
    b.frame_times(False)                        # allowed again
    # a streaming batch cannot switch it on
    s = ReceiverBatch(2)
    s.stream_nmea()
    state_error(s.unique, 128)


def delayed(make, n_ch, delays):
    return np.stack([np.roll(make(c), delays[c], axis=0) for c in range(n_ch)], axis=1)


def test_iq_input_with_the_afc():
    n_ch, total = 6, 12 * 1280
    prng = np.random.default_rng(9)
    pay = [synth.random_position_report(prng) for _ in range(9)]
    x = delayed(lambda c: synth.make_iq_stream(total, seed=3, channel=c, sigma=800.0, gated=True, offset_hz=3000.0,
                                               payloads=lambda rng, slot: pay[slot] if slot < len(pay) else None)[0],
                n_ch, ur.DELAYS6)
    b, t = pair(n_ch, 128, max_len=8192)
    for r in (b, t):
        r.afc(1024)
    ck = Check(b, t, 128)
    xd = dev(x)
    for a, e in [(0, 1020), (1020, 1021), (1021, 5117), (5117, 12000), (12000, total)]:
        b.run_iq(xd[a:e])
        t.run_iq(xd[a:e])
        if e == 5117:
            ck.drain()
    got = ck.drain()
    assert ck.twin_frames > 40 and ck.records <= 9 and got[2].max() >= 5


def test_wideband_input_two_streams_of_two_offsets():
    M, D, offs = 2, 6, (-25000, 25000)
    n = 12 * 1280 * D
    base = synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=0, amplitude=1500.0, sigma=0.0, occupancy=0.8,
                                      gated=True)[0].astype(np.float64)
    rng = np.random.default_rng(10)
    x = np.stack([np.roll(base, 17 * D * s, axis=0) + rng.normal(0.0, 225.0, base.shape) for s in range(M)], axis=1)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    N = M * len(offs)
    b, t = pair(N, 128, max_len=8192)
    for r in (b, t):
        r.channeliser(D, 48000 * D, offs)
    ck = Check(b, t, 128)
    xd = dev(x)
    cuts = [0, D * 1020, D * 1021, D * 5117, D * 9000, n]
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run_wideband(xd[a:e])
        t.run_wideband(xd[a:e])
        if e == D * 5117:
            ck.drain()
    got = ck.drain()
    assert ck.twin_frames > 20 and ck.records < ck.twin_frames and got[2].max() == 2


def test_a_node_merges_copies_that_lie_on_different_shards():
    from gnuais_amd.shard import ReceiverNode
    x = ur.receivers(1, ur.DELAYS6)
    nd, tw = (ReceiverNode(6, devices=[0, 0], max_len=ur.TOTAL) for _ in range(2))
    assert [s[2] for s in nd.shards] == [3, 3]
    with pytest.raises(GnuaisError) as e:
        nd.unique(128)                          # the node does not time its frames yet
    assert e.value.code == E_STATE
    for r in (nd, tw):
        r.frame_times(True)
    nd.unique(128)
    ref = ur.UniqueRef(128)
    cuts = ur.ragged_cuts()
    n_rec = n_twin = copies = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        for r in (nd, tw):
            r.run_host(x[a:e])
            r.sync()
        got = nd.drain_frames_unique()
        fr, tm = tw.drain_frames_timed()
        want = ref.push(fr, tm, int(e))
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert nd.unique_late() == ref.late
        n_rec, n_twin, copies = n_rec + len(got[0]), n_twin + len(fr), copies + int(got[2].sum())
    assert n_twin == 48 and n_rec == 8 and copies + nd.unique_late() == 48
    nd.reset()
    assert nd.unique_late() == 0
    nd.close()
    tw.close()


def test_one_larger_shape():
    """4096 channels x 48 000 rows: 16 base streams, each on 256 channels with delays (c // 16) % 40, built on the
    device"""
    import torch
    n_ch, total = 4096, 48000
    base, _ = synth.make_base_streams(16, total, seed=7, occupancy=0.8)
    bt = dev(base)                                              # [16][total]
    x = torch.empty((total, n_ch), dtype=torch.int16, device=bt.device)
    ch = torch.arange(n_ch, device=bt.device)
    for d in range(40):
        cols = ch[(ch // 16) % 40 == d]
        x[:, cols] = torch.roll(bt[cols % 16], d, dims=1).t()
    b, t = pair(n_ch, 128, max_len=total)
    ck = Check(b, t, 128)
    for r in (b, t):
        r.run(x)
    got = ck.drain()
    # a stream is on 256 channels: no cluster can be larger, and most of a stream's receivers decode each frame
    assert ck.twin_frames > 50000 and 200 < got[2].max() <= 256 and ck.records < ck.twin_frames // 100
