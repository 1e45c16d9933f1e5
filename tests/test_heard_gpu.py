"""Who heard each transmission on the device (gnuais_batch_drain_frames_heard, frame_unique.hip).  The expected value is
always tests/heard_ref.py applied to what drain_frames_signal() -- or drain_frames_timed(), while the signal feature is
off -- of a TWIN batch gives for the same calls, so the new drain is never compared with itself.  The shapes are those
of test_unique_gpu.py: the smallest at which the stage can go wrong."""
import ctypes as C

import numpy as np
import pytest

import heard_ref as hr
import unique_ref as ur
from gnuais_amd import synth
from gnuais_amd.lib import E_ARG, FRAME_DTYPE, HEARER_DTYPE, SIGNAL_DTYPE
from test_iq_gpu import dev
from test_repair_gpu import crafted_payload, flipped_frame
from test_unique_gpu import GAP, late_input, slots_stream, square, three_payloads

pytestmark = pytest.mark.gpu


def pair(n_ch, W, max_len=ur.TOTAL, repair=False, hash_bits=64, signal=False, setup=None):
    """the batch under test and its twin, which only times (and measures) its frames"""
    from gnuais_amd import ReceiverBatch
    b, t = ReceiverBatch(n_ch, max_len=max_len), ReceiverBatch(n_ch, max_len=max_len)
    for x in (b, t):
        if repair:
            x.repair(True)
        if setup:
            setup(x)
        x.frame_times(True)
        if signal:
            x.frame_signal(True)
    b.unique(W)
    if hash_bits != 64:
        b.set_option("unique_hash_bits", hash_bits)
    return b, t


class Check:
    """drain by drain: the heard (or, with heard=False, the unique) drain of `b` against the restatement over the twin's
    signal or timed drain"""

    def __init__(self, b, t, W, signal=False):
        self.b, self.t, self.ref, self.signal = b, t, hr.HeardRef(W), signal
        self.twin_frames = self.listed = self.records = 0
        self.twin_signal = {}           # (channel, t) -> the twin's record

    def drain(self, heard=True):
        got = self.b.drain_frames_heard() if heard else self.b.drain_frames_unique()
        if self.signal:
            fr, tm, sg = self.t.drain_frames_signal()
        else:
            (fr, tm), sg = self.t.drain_frames_timed(), None
        rows = int(self.t.info("rows"))
        assert rows == int(self.b.info("rows"))
        want = self.ref.push_heard(fr, tm, rows, signal=sg) if heard else self.ref.push(fr, tm, rows)
        assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]), len(fr))
        assert got[0].tobytes() == want[0].tobytes()
        assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int64
        assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32, (got[2], want[2])
        if heard:
            assert np.array_equal(got[3], want[3]) and got[3].dtype == np.int32, (got[3], want[3])
            assert got[4].dtype == HEARER_DTYPE and got[4].tobytes() == want[4].tobytes(), np.argwhere(got[4] != want[4])[:5]
            hr.check_invariants(*got)
            if sg is None:
                assert not got[4]["signal"].tobytes().strip(b"\0")
            else:
                for f, t, s in zip(fr, tm, sg):
                    self.twin_signal[(int(f["channel"]), int(t))] = s
                for m in got[4]:
                    assert m["signal"] == self.twin_signal[(int(m["channel"]), int(m["t"]))]
        assert self.b.unique_late() == self.ref.late
        self.twin_frames += len(fr)
        self.listed += len(got[4]) if heard else int(got[2].sum())
        self.records += len(got[0])
        assert self.listed + self.b.unique_late() == self.twin_frames
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
        assert got[2].tolist() == [6] * 8 and got[3].tolist() == list(range(0, 49, 6)) and b.unique_late() == 0
        assert got[4]["channel"].tolist() == list(range(6)) * 8       # the delays grow with the channel


@pytest.mark.parametrize("hash_bits", [64, 1, 3])
@pytest.mark.parametrize("per_call", [False, True])
def test_seventy_receivers_and_forced_hash_collisions(seventy, per_call, hash_bits):
    """10 groups x 7 delays; with the hash cut to 1 and 3 bits the exact path gives the same lists"""
    b, t = pair(70, 128, hash_bits=hash_bits)
    ck = Check(b, t, 128)
    run_calls(b, t, seventy, ur.ragged_cuts(), ck.drain if per_call else None)
    got = ck.drain()
    assert ck.twin_frames > 500 and 80 <= ck.records <= 90
    if not per_call:
        assert got[2].max() == 7 and np.count_nonzero(got[2] == 7) > 60 and len(got[4]) == ck.twin_frames


def test_a_cluster_wider_than_a_workgroup():
    """300 channels carry one payload stream, delays c % 41: a cluster's members cross a workgroup, and the differences
    of `first` exceed 256"""
    one = ur.receivers(1, [0])[:, 0]
    rng = np.random.default_rng(5)
    x = np.stack([np.roll(one, c % 41) for c in range(300)], axis=1).astype(np.int32)
    x = np.clip(x + rng.normal(0.0, 300.0, x.shape).round().astype(np.int32), -32768, 32767).astype(np.int16)
    b, t = pair(300, 128)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, ur.TOTAL])
    got = ck.drain()
    assert ck.records == 8 and np.count_nonzero(np.diff(got[3]) > 256) >= 6 and got[2].max() == 300


@pytest.mark.parametrize("W,clusters", [(1300, 1), (1200, 8)])
def test_a_chain_of_copies_one_slot_apart(W, clusters):
    p = synth.random_position_report(np.random.default_rng(1))
    x = np.stack([slots_stream(ur.TOTAL, {s: p for s in range(8) if s % 2 == c}, channel=c) for c in range(2)], axis=1)
    b, t = pair(2, W)
    ck = Check(b, t, W)
    run_calls(b, t, x, [0, ur.TOTAL])
    got = ck.drain()
    assert ck.twin_frames == 8 and got[2].tolist() == [8 // clusters] * clusters
    assert got[4]["channel"].tolist() == [0, 1] * 4 and np.all(np.diff(got[4]["t"]) > 1200)


def test_late_copies_across_a_drain():
    """delays 0 and 600, W = 700, the cut between the ends of the two copies: the second drain lists nothing for the
    transmission and counts one late copy"""
    x = late_input([0, 600])
    b, t = pair(2, 700)
    ck = Check(b, t, 700)
    xd = dev(x)
    for (a, e), (n_rec, late) in zip([(0, 2800), (2800, 5000), (5000, ur.TOTAL)], [(1, 0), (0, 1), (1, 1)]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        got = ck.drain()
        assert len(got[0]) == n_rec and b.unique_late() == late, (a, e, len(got[0]), b.unique_late())
        assert got[3].tolist() == list(range(n_rec + 1)) and len(got[4]) == n_rec
        assert got[4]["channel"].tolist() == [0] * n_rec
    assert ck.twin_frames == 3


@pytest.mark.parametrize("both_damaged", [False, True])
def test_the_intact_copy_is_the_primary_and_every_member_has_its_own_flags(both_damaged):
    payload = crafted_payload(np.random.default_rng(4), 21)
    bad, good = flipped_frame(payload, 30), synth.hdlc_frame_bits(payload).tolist()
    x = np.stack([square(bad, 100, 2048), square(bad if both_damaged else good, 120, 2048)], axis=1)
    b, t = pair(2, 128, max_len=2048, repair=True)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, 2048])
    f, tm, c, first, m = ck.drain()
    assert ck.twin_frames == 2 and c.tolist() == [2] and first.tolist() == [0, 2]
    assert m["channel"].tolist() == [0, 1] and m["t"][0] < m["t"][1]
    assert [bool(x & ur.REPAIRED) for x in m["flags"].tolist()] == [True, both_damaged]
    assert int(f[0]["channel"]) == (0 if both_damaged else 1)


def test_untimed_frames_are_clusters_of_one_member():
    n_ch = 5
    rng = np.random.default_rng(8)
    pay = [synth.random_position_report(rng) for _ in range(2)]
    streams = [np.array(GAP + synth.hdlc_frame_bits(pay[c % 2]).tolist() + GAP + synth.hdlc_frame_bits(pay[0]).tolist() + GAP,
                        dtype=np.uint8) for c in range(n_ch)]
    b, t = pair(n_ch, 128, max_len=2048)
    ck = Check(b, t, 128)
    b.decode_bits(streams)
    t.decode_bits(streams)
    f, tm, c, first, m = ck.drain()             # a drain that holds only t = -1 frames
    assert len(f) == 2 * n_ch and np.all(m["t"] == -1) and first.tolist() == list(range(2 * n_ch + 1))
    assert m["channel"].tolist() == f["channel"].tolist() and m["flags"].tolist() == f["flags"].tolist()
    b.decode_bits(streams)
    t.decode_bits(streams)
    run_calls(b, t, three_payloads(n_ch), [0, 2048])
    f, tm, c, first, m = ck.drain()             # mixed: the untimed ones first
    assert np.all(m["t"][: 2 * n_ch] == -1) and np.all(m["t"][2 * n_ch:] >= 0) and len(m) == 3 * n_ch


@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 257])
def test_drains_of_a_chosen_number_of_frames(n_ch):
    b, t = pair(n_ch, 128, max_len=2048)
    ck = Check(b, t, 128)
    got = ck.drain()                            # a drain of 0 frames
    assert [len(x) for x in got] == [0, 0, 0, 1, 0] and got[3].tolist() == [0] and got[4].dtype == HEARER_DTYPE
    run_calls(b, t, three_payloads(n_ch), [0, 2048])
    got = ck.drain()
    assert ck.twin_frames == n_ch and ck.records == min(n_ch, 3) and len(got[4]) == n_ch
    assert sorted(got[4]["channel"].tolist()) == list(range(n_ch))


def test_the_two_drains_alternate_on_one_batch_against_one_restatement(seventy):
    b, t = pair(70, 128)
    ck = Check(b, t, 128)
    turn = [0]

    def each():
        ck.drain(heard=turn[0] % 2 == 0)
        turn[0] += 1
    run_calls(b, t, seventy, ur.ragged_cuts(), each)
    ck.drain(heard=False)
    assert ck.twin_frames > 500 and 80 <= ck.records <= 90 and turn[0] == len(ur.ragged_cuts()) - 1


def iq_receivers(n_ch, total, offset_hz=3000.0):
    prng = np.random.default_rng(9)
    pay = [synth.random_position_report(prng) for _ in range(9)]
    return np.stack([np.roll(synth.make_iq_stream(total, seed=3, channel=c, sigma=800.0, gated=True, offset_hz=offset_hz,
                                                  payloads=lambda rng, slot: pay[slot] if slot < len(pay) else None)[0],
                             ur.DELAYS6[c], axis=0) for c in range(n_ch)], axis=1)


@pytest.mark.parametrize("signal", [True, False])
def test_iq_input_every_member_carries_the_twins_record(signal):
    """run_iq with the AFC: with gnuais_batch_frame_signal on, every member's record is the twin's for that (channel, t)
    (Check.drain asserts it member by member); with it off the records are zeros"""
    n_ch, total = 6, 12 * 1280
    x = iq_receivers(n_ch, total)
    b, t = pair(n_ch, 128, max_len=8192, signal=signal, setup=lambda r: r.afc(1024))
    ck = Check(b, t, 128, signal=signal)
    xd = dev(x)
    for a, e in [(0, 1020), (1020, 1021), (1021, 5117), (5117, 12000), (12000, total)]:
        b.run_iq(xd[a:e])
        t.run_iq(xd[a:e])
        if e == 5117:
            ck.drain()
    got = ck.drain()
    assert ck.twin_frames > 40 and ck.records <= 9 and got[2].max() >= 5
    measured = np.count_nonzero(got[4]["signal"]["blocks"])
    assert measured > 20 if signal else measured == 0


def test_wideband_input_two_streams_of_two_offsets():
    M, D, offs = 2, 6, (-25000, 25000)
    n = 12 * 1280 * D
    base = synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=0, amplitude=1500.0, sigma=0.0, occupancy=0.8,
                                      gated=True)[0].astype(np.float64)
    rng = np.random.default_rng(10)
    x = np.stack([np.roll(base, 17 * D * s, axis=0) + rng.normal(0.0, 225.0, base.shape) for s in range(M)], axis=1)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    N = M * len(offs)
    b, t = pair(N, 128, max_len=8192, signal=True, setup=lambda r: r.channeliser(D, 48000 * D, offs))
    ck = Check(b, t, 128, signal=True)
    xd = dev(x)
    cuts = [0, D * 1020, D * 1021, D * 5117, D * 9000, n]
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run_wideband(xd[a:e])
        t.run_wideband(xd[a:e])
        if e == D * 5117:
            ck.drain()
    got = ck.drain()
    assert ck.twin_frames > 20 and ck.records < ck.twin_frames and got[2].max() == 2
    assert np.count_nonzero(got[4]["signal"]["blocks"]) > 10


@pytest.mark.parametrize("signal", [True, False])
def test_a_node_equals_the_unsharded_batch_with_copies_on_different_shards(signal):
    """two shards of three channels; the six receivers' copies of a transmission lie on both.  The node's lists (host
    merge over the shards' signal or timed drains, global channel numbers) are the unsharded batch's (device)."""
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.shard import ReceiverNode
    total = 10 * 1280
    x = iq_receivers(6, total, offset_hz=0.0) if signal else ur.receivers(1, ur.DELAYS6)
    nd = ReceiverNode(6, devices=[0, 0], max_len=4096)
    b = ReceiverBatch(6, max_len=4096)
    assert [s[2] for s in nd.shards] == [3, 3]
    for r in (nd, b):
        r.frame_times(True)
        if signal:
            r.frame_signal(True)
        r.unique(128)
    n_rec = listed = measured = 0
    for a in range(0, total, 4096):
        seg = x[a:a + 4096]
        if signal:
            nd.run_iq_host(seg)
            b.run_iq(dev(seg))
        else:
            nd.run_host(seg)
            b.run(dev(seg))
        nd.sync()
        got, want = nd.drain_frames_heard(), b.drain_frames_heard()
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
        hr.check_invariants(*got)
        assert nd.unique_late() == b.unique_late()
        n_rec, listed = n_rec + len(got[0]), listed + len(got[4])
        measured += int(np.count_nonzero(got[4]["signal"]["blocks"]))
        for i in range(len(got[0])):            # the copies of a cluster come from both shards
            if got[2][i] == 6:
                assert set((got[4]["channel"][got[3][i]:got[3][i + 1]] // 3).tolist()) == {0, 1}
    assert n_rec >= 7 and listed + nd.unique_late() >= 40
    assert measured > 20 if signal else measured == 0
    nd.close()


def test_max_too_small_consumes_nothing():
    x = ur.receivers(1, ur.DELAYS6)
    b, t = pair(6, 128)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, ur.TOTAL])
    n = b.pending_frames()
    assert n == 48
    out, tms, cps = np.zeros(n, dtype=FRAME_DTYPE), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    first, mem = np.full(n + 1, 7, dtype=np.int32), np.zeros(n, dtype=HEARER_DTYPE)
    got, nm = C.c_int(-1), C.c_int(-1)
    rc = b._lib.gnuais_batch_drain_frames_heard(b._h, out.ctypes.data, tms.ctypes.data, cps.ctypes.data, n - 1, C.byref(got),
                                                first.ctypes.data, mem.ctypes.data, C.byref(nm))
    assert rc == E_ARG and got.value == 0 and nm.value == 0 and first[0] == 0 and b.pending_frames() == n
    got = ck.drain()
    assert got[2].tolist() == [6] * 8 and len(got[4]) == 48 and SIGNAL_DTYPE == HEARER_DTYPE.fields["signal"][0]
