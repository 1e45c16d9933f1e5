"""The long frames' signal records and cover on the device (gnuais_batch_long_frame_signal, long_signal.hip).  Every
comparison is byte for byte against the restatement tests/long_signal_ref.py (tests/test_long_signal_cpu.py shows that it
is not empty).  Every test keeps a twin batch that gets the same calls with the feature off and every other feature as
the test has it: its chain state, long records, counters and short frames' signal records must be the same."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chan_ref
import heard_ref as hr
import iq_ref
import long_ref as lr
import long_signal_ref as lsr
import resample_ref as rr
from gnuais_amd import params, synth
from gnuais_amd.lib import E_STATE, HEARER_DTYPE, SIGNAL_DTYPE, GnuaisError
from test_frame_signal_gpu import Front
from test_iq_gpu import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
PLLINC = 0x10000 // 5


def chain_state(b):
    return (b.counters().tobytes(), b.fsm_state().tobytes(), b.pll_state().tobytes(), b.long_fsm_state().tobytes())


def counters3(b):
    d, f = b.long_counters()
    return np.stack([d, f, b.long_repaired()], axis=1)


class Rig:
    """a batch with the feature on, its twin with it off, and the restatement, fed the same calls"""

    def __init__(self, n_ch, max_len, taps=None, pllinc=0, W=0, repair=False, variant=None, nbuf=None, configure=None,
                 feature=True):
        from gnuais_amd import ReceiverBatch
        kw = {} if taps is None else dict(taps=taps, pllinc=pllinc)
        self.on, self.off = ReceiverBatch(n_ch, max_len=max_len, **kw), ReceiverBatch(n_ch, max_len=max_len, **kw)
        for b in (self.on, self.off):
            if variant is not None:
                b.set_option("pll_variant", variant)
            if nbuf is not None:
                b.set_option("nbuf", nbuf)
            if W:
                b.afc(W)
            if configure:
                configure(b)
            b.frame_times(True)
            b.frame_signal(True)
            b.long_frames(True)
            if repair:
                b.long_repair(True)
            assert b.info("long_frame_signal") == 0
        self.ref, self.front = lsr.LongSignalRef(n_ch, taps, pllinc, W, repair), Front(n_ch, W)
        self.ref.fs.switch_on()
        if feature:
            self.on.long_frame_signal(True)
            assert self.on.info("long_frame_signal") == 1 and self.off.info("long_frame_signal") == 0
            self.ref.long_switch_on()

    def iq(self, seg):
        """an I/Q-type call of the rows seg [len][n_ch][2]"""
        d = dev(seg)
        self.on.run_iq(d, sync=False)
        self.off.run_iq(d, sync=False)
        self.ref.run_iq(seg, self.front.audio(seg))

    def wide(self, seg, iq):
        """a wideband call of the wide samples seg, whose wide stage gives the pairs iq"""
        d = dev(seg)
        self.on.run_wideband(d, sync=False)
        self.off.run_wideband(d, sync=False)
        self.ref.run_iq(iq, self.front.audio(iq))

    def audio(self, a):
        d = dev(a)
        self.on.run(d, sync=False)
        self.off.run(d, sync=False)
        self.ref.run_audio(a)

    def bits(self, per_channel):
        self.on.decode_bits(per_channel)
        self.off.decode_bits(per_channel)
        self.ref.decode_bits(per_channel)

    def check(self):
        """one drain against the restatement and the twin: -> (long records, their signal records)"""
        rec, sig = self.on.drain_long_frames_signal()
        wrec, wsig = self.ref.drain_long()
        assert rec.tobytes() == wrec.tobytes(), (len(rec), len(wrec))
        assert sig.dtype == SIGNAL_DTYPE and sig.tobytes() == wsig.tobytes(), (sig.tolist(), wsig.tolist())
        assert self.off.drain_long_frames().tobytes() == rec.tobytes()
        self.check_short()
        return rec, sig

    def check_short(self):
        """the short frames, their times and records, and the chain's state: the restatement's and the twin's"""
        fr, t, s = self.on.drain_frames_signal()
        tf, tt, ts = self.off.drain_frames_signal()
        wf, wt, ws = self.ref.drain()
        assert fr.tobytes() == tf.tobytes() == wf.tobytes() and np.array_equal(t, tt) and np.array_equal(t, wt)
        assert s.tobytes() == ts.tobytes() == ws.tobytes()
        assert chain_state(self.on) == chain_state(self.off) and np.array_equal(counters3(self.on), counters3(self.off))


# ---- 1. LS9 on two channels, ragged calls, the ring gone round ------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 8])
@pytest.mark.parametrize("max_len", [5000, 2048])
def test_ls9_ragged_calls_equal_the_restatement(max_len, variant):
    """calls of (4096, 1, 2047, 5000) rows, cut to max_len; with max_len 2048 the signal ring (5 calls of 2048 rows, the
    1008-bit span and the widest AFC window: 371 blocks) goes round more than twice under the 960 blocks of the input;
    one drain in the middle"""
    x = lsr.ls9()
    pattern = tuple(min(n, max_len) for n in lsr.LS9_CALLS)
    rig = Rig(2, max_len, variant=variant)
    calls = lsr.ragged(lsr.LS9_ROWS, pattern)
    got = []
    for i, (a, e) in enumerate(calls):
        rig.iq(x[a:e])
        if i == len(calls) // 2:
            got.append(rig.check())
    got.append(rig.check())
    rec = np.concatenate([g[0] for g in got])
    sig = np.concatenate([g[1] for g in got])
    assert len(got[0][0]) >= 2 and len(got[1][0]) >= 2
    assert sorted(rec["nbits"].tolist()) == sorted([432, 480, 640, 800, 1008] * 2)
    assert sorted(sig["blocks"].tolist()) == sorted([35, 39, 51, 63, 79] * 2)
    if max_len == 5000:                                     # the drains' records together are the one drain's of the shared restatement
        want = lsr.ls9_restated()
        order = np.lexsort((rec["t"], rec["channel"]))
        assert rec[order].tobytes() == want["long"].tobytes() and sig[order].tobytes() == want["long_sig"].tobytes()


# ---- 2. the wave geometry ----------------------------------------------------------------------------------------------
def test_seventy_channels_every_t_mod_64_and_63_64_65_79_blocks():
    """bursts of 800, 816 and 1008 bits on 70 channels, channel c turned by 7 c rows: every t mod 64 occurs, a call closes
    more long frames than a workgroup has waves, nb takes 63, 64, 65 and 79 / 80"""
    n_ch, total = 70, 18 * 1280
    base = synth.make_iq_stream(total, seed=9, channel=0, sigma=800.0, amplitude=10000.0, gated=True,
                                payloads=lr.long_payloads(sizes=(100, 102, 126)))[0]
    x = np.stack([np.roll(base, 7 * c, axis=0) for c in range(n_ch)], axis=1)
    rig = Rig(n_ch, 8192)
    for a in range(0, total, 8192):
        rig.iq(x[a:a + 8192])
    rec, sig = rig.check()
    assert len(rec) > 2 * n_ch and len(set((rec["t"] % 64).tolist())) == 64      # (some turns lose the first burst)
    per_call = np.bincount(rec["t"] // 8192)
    assert per_call.max() >= n_ch > 64
    blocks = set(sig["blocks"].tolist())
    assert {63, 64, 65, 79} <= blocks, blocks


# ---- 3. the (0, 0, 0) cases ----------------------------------------------------------------------------------------------
def test_zero_records_late_switch_audio_call_decode_bits_reset_and_switched_off():
    x = lsr.ls9()
    audio = iq_ref.discriminate(x, None)[0]
    rig = Rig(2, 9000, feature=False)
    rig.iq(x[:1500])                                        # inside the first burst (t = 2535, its span begins near row 200)
    rig.check_short()
    rig.on.long_frame_signal(True)
    rig.off.frame_signal(True)                              # the twin starts a new run at the same row
    rig.ref.long_switch_on()
    rig.iq(x[1500:9000])
    rec, sig = rig.check()
    assert len(rec) == 2 and not sig["blocks"].any()        # switched on inside the burst: its span reaches behind v0
    rig.iq(x[9000:12000])                                   # the second burst (t = 10472)
    rec, sig = rig.check()
    assert rec["nbits"].tolist() == [480, 480] and sig["blocks"].tolist() == [39, 39]
    rig.iq(x[12000:18000])
    rig.audio(audio[18000:19500])                           # an audio-type call closes the third burst (t = 18928)
    rig.iq(x[19500:24000])
    rec, sig = rig.check()
    assert rec["nbits"].tolist() == [640, 640] and not sig["blocks"].any()
    rig.iq(x[24000:30000])                                  # the fourth: measured, the run began at row 19500
    rec, sig = rig.check()
    assert rec["nbits"].tolist() == [800, 800] and sig["blocks"].tolist() == [63, 63]
    one = np.concatenate([lr.burst(np.random.default_rng(5).integers(0, 256, 60, dtype=np.uint8)), np.zeros(3, dtype=np.uint8)])
    rig.bits([one, one])                                    # bits without samples: t = -1
    rec, sig = rig.check()
    assert rec["t"].tolist() == [-1, -1] and rec["nbits"].tolist() == [480, 480] and not sig.view(np.uint64).any()
    # a record appended while the switch was off
    rig.on.long_frame_signal(False)
    rig.ref.long_switch_off()
    with pytest.raises(GnuaisError) as e:
        rig.on.drain_long_frames_signal()
    assert e.value.code == E_STATE
    rig.iq(x[30000:38000])                                  # the fifth burst (t = 36171) closes unmeasured
    rig.check_short()
    rig.on.long_frame_signal(True)
    rig.off.frame_signal(True)
    rig.ref.long_switch_on()
    rec, sig = rig.check()
    assert rec["nbits"].tolist() == [1008, 1008] and not sig.view(np.uint64).any()
    # a reset: the run starts at row 0, the first burst is measured
    for b in (rig.on, rig.off):
        b.reset()
    rig.ref.reset()
    rig.front.reset()
    assert rig.on.info("long_frame_signal") == 1 and rig.on.info("rows") == 0
    rig.iq(x[:9000])
    rec, sig = rig.check()
    assert rec["t"].tolist() == [2535, 2536] and sig["blocks"].tolist() == [35, 35]


# ---- 4. a repaired long frame --------------------------------------------------------------------------------------------
def test_repaired_long_frames_carry_the_record_of_their_own_length():
    """100-byte bursts at the amplitude and noise of tests/test_frame_signal_gpu.py's repaired case: most fail their CRC
    by one symbol and are repaired; a repaired record is measured over n' bits from the candidate's t"""
    n_ch, total = 8, 4 * 6 * 1280
    x = np.stack([synth.make_iq_stream(total, seed=20, channel=c, sigma=700.0, amplitude=3000.0, gated=True,
                                       payloads=lr.long_payloads(sizes=(100, 100, 100, 100)))[0] for c in range(n_ch)], axis=1)
    rig = Rig(n_ch, 8192, repair=True)
    for a in range(0, total, 8192):
        rig.iq(x[a:a + 8192])
    rec, sig = rig.check()
    rep = (rec["flags"] & 0x40) != 0
    assert rep.sum() >= 1 and rep.sum() == rig.on.long_repaired().sum() and (~rep).sum() >= 1
    assert np.all(rec["nbits"][rep] == 800) and np.all(sig["blocks"][rep] >= 63)


# ---- 5. the AFC --------------------------------------------------------------------------------------------------------
def test_afc_window_1024_moves_q_by_half_a_window():
    x = lsr.ls9()[:30000]
    rig = Rig(2, 8192, W=1024)
    for a in range(0, len(x), 8192):
        rig.iq(x[a:a + 8192])
    rec, sig = rig.check()
    assert len(rec) >= 6 and np.all(sig["blocks"] > 0)
    plain = lsr.ls9_restated()["long"]
    assert np.all(rec["t"][:3] - plain["t"][:3] >= 500)      # the same bursts close half a window later


# ---- 6. the 192 kHz table ------------------------------------------------------------------------------------------------
def test_192k_table_a_lane_takes_several_rounds():
    n_ch, sps = 2, 20
    total = 12 * synth.SLOT_BITS * sps
    x = np.stack([synth.make_iq_stream(total, seed=9, channel=c, sps=sps, sigma=800.0, amplitude=10000.0, gated=True,
                                       rate_hz=9600 * sps, payloads=lr.long_payloads(sizes=(54, 126)))[0]
                  for c in range(n_ch)], axis=1)
    calls = [1, 777, 2049, 12000]
    rig = Rig(n_ch, 12000, taps=params.taps_192k(), pllinc=params.PLLINC_192K)
    pos, i = 0, 0
    while pos < total:
        n = min(calls[min(i, 3)], total - pos)
        rig.iq(x[pos:pos + n])
        pos, i = pos + n, i + 1
    rec, sig = rig.check()
    assert sorted(rec["nbits"].tolist()) == [432, 432, 1008, 1008]
    assert np.all(sig["blocks"][rec["nbits"] == 1008] > 256) and np.all(sig["blocks"][rec["nbits"] == 432] > 128)


# ---- 7. wideband input -----------------------------------------------------------------------------------------------------
def test_wideband_integer_ratio():
    M, D, offs = 2, 6, (-25000, 25000)
    N, n = M * len(offs), 12 * 1280 * D
    x = np.stack([synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=s, amplitude=1500.0, sigma=225.0,
                                             gated=True, payloads=lr.long_payloads(sizes=(60, 126)))[0] for s in range(M)], axis=1)
    calls = [D * 1020, D, D * 4096, D * 333]
    calls.append(n - sum(calls))
    rig = Rig(N, max(calls) // D, configure=lambda b: b.channeliser(D, 48000 * D, offs))
    ch = chan_ref.Channeliser(M, D, 48000 * D, offs)
    pos = 0
    for c in calls:
        rig.wide(x[pos:pos + c], ch.run(x[pos:pos + c]))
        pos += c
    rec, sig = rig.check()
    assert len(rec) == 8 and np.all(sig["blocks"] > 0) and sig["blocks"].max() >= 79


def test_wideband_resampler_3_64():
    up, down, M, offs = 3, 64, 2, [-25000, 25000]
    N, rate = M * len(offs), 48000 * down // up
    n = 12 * 1280 * down // up
    x = np.stack([synth.make_resampled_wideband_stream(n, up, down, (-25000, 25000), seed=5, stream=s, sigma=300.0, gated=True,
                                                       payloads=lr.long_payloads(sizes=(60, 126)))[0] for s in range(M)], axis=1)
    periods = n // down
    cuts = [0, 1, periods // 8, periods // 8 + 1, periods // 3, periods]
    rows = max(b - a for a, b in zip(cuts[:-1], cuts[1:])) * up
    rig = Rig(N, rows, configure=lambda b: b.resampler(up, down, rate, offs))
    r = rr.Resampler(M, up, down, rate, offs)
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = x[a * down:e * down]
        rig.wide(seg, r.run(seg))
    rec, sig = rig.check()
    assert len(rec) == 8 and np.all(sig["blocks"] > 0) and sig["blocks"].max() >= 79


# ---- 8. the channel load -------------------------------------------------------------------------------------------------
OCC_CALLS = (4096, 1, 2047, 16384)


def occ_check(b, want, E=64, tap=True):
    """the batch's final epochs against the restatement's: first blocks, records, tap words (tap: where the code ring
    still holds every epoch); -> (covered, busy) in total"""
    first, rec = b.drain_occupancy()
    assert first.tolist() == [w[0] for w in want], (first.tolist(), [w[0] for w in want])
    for k, (f0, wrec, words) in enumerate(want):
        assert rec[k].tobytes() == wrec.tobytes(), (f0, rec[k], wrec)
        if tap:
            got = b.occupancy_blocks(f0, E)
            assert np.array_equal(got, words), (f0, np.argwhere(got != words)[:5])
    return int(rec["covered"].sum()), int(rec["busy"].sum())


def test_occupancy_on_ls9_the_long_frames_cover_their_air_time():
    """E = 64, margin 16, calls of (4096, 1, 2047, 16384): one tail makes four epochs final.  The twin switched occupancy
    on with the feature off: its LAG, epochs and records are those of occupancy_ref unchanged"""
    x = lsr.ls9()
    rig = Rig(2, 16384)
    assert rig.on.info("occupancy_lag") == 5562 and rig.off.info("occupancy_lag") == 2762
    for b in (rig.on, rig.off):
        b.occupancy(64, 16)
    assert rig.on.info("occupancy_lag") == 5562 and rig.off.info("occupancy_lag") == 2762
    finals = []
    for a, e in lsr.ragged(lsr.LS9_ROWS, OCC_CALLS):
        before = (max(a - 5562, 0)) // 4096, max(e - 5562, 0) // 4096
        finals.append(before[1] - before[0])
        rig.iq(x[a:e])
    assert max(finals) >= 4
    want_on = lsr.ls9_epochs(True, pattern=OCC_CALLS)
    want_off = lsr.ls9_epochs(False, pattern=OCC_CALLS)
    assert len(want_on) == (lsr.LS9_ROWS - 5562) // 4096 == 13 and len(want_off) == 14
    cov_on, busy_on = occ_check(rig.on, want_on)
    cov_off, busy_off = occ_check(rig.off, want_off)
    print("covered", cov_on, "of", busy_on, "; the twin", cov_off, "of", busy_off)
    assert cov_on > cov_off and cov_on >= 4 * 78
    # leaving the long cover out gives other records: the restatement with the long LAG and the short frames alone
    r = lsr.ls9_restated(OCC_CALLS)
    occ = lsr.LongOccupancyRef(2, 64, 16)
    for a, e in lsr.ragged(lsr.LS9_ROWS, OCC_CALLS):
        occ.run_iq(a, x[a:e])
    occ.add_frames(r["short"], r["short_t"])
    assert sum(int(w[1]["covered"].sum()) for w in occ.epochs()) < cov_on
    rig.check()


# ---- 9. who heard the long bursts, and how strongly ---------------------------------------------------------------------
AMPLITUDES = (4000.0, 10000.0, 16000.0)


def heard_input():
    """three receivers hear the same three long bursts at three levels (the loudest loses the second: eight records)"""
    total = 18 * 1280
    return np.stack([synth.make_iq_stream(total, seed=9, channel=c, sigma=400.0, amplitude=a, gated=True,
                                          payloads=lr.long_payloads(sizes=(54, 100, 126)))[0]
                     for c, a in enumerate(AMPLITUDES)], axis=1)


def test_heard_members_carry_each_copys_record():
    from gnuais_amd.receiver import LongUniq
    x, W = heard_input(), 64
    rig = Rig(3, 8192)
    from gnuais_amd import ReceiverBatch
    plain = ReceiverBatch(3, max_len=8192)                  # the same batch again, drained plainly
    plain.frame_times(True)
    plain.frame_signal(True)
    plain.long_frames(True)
    plain.long_frame_signal(True)
    rig.on.long_unique(W)
    rig.off.long_unique(W)
    for a in range(0, len(x), 8192):
        rig.iq(x[a:a + 8192])
        plain.run_iq(dev(x[a:a + 8192]), sync=False)
    prec, psig = plain.drain_long_frames_signal()
    wrec, wsig = rig.ref.drain_long()
    assert prec.tobytes() == wrec.tobytes() and psig.tobytes() == wsig.tobytes() and len(prec) == 8
    rows = int(rig.on.info("rows"))
    rec, copies, first, members = rig.on.drain_long_frames_heard()
    assert members.dtype == HEARER_DTYPE and copies.tolist() == [3, 2, 3]
    by = {(int(r["channel"]), int(r["t"])): s for r, s in zip(prec, psig)}
    for m in members:                                       # the plain drain's record of the same copy
        assert m["signal"].tobytes() == by[(int(m["channel"]), int(m["t"]))].tobytes() and m["signal"]["blocks"] > 0
    for i in range(3):                                      # the levels lie as far apart as the amplitudes
        ms = sorted(members[first[i]:first[i + 1]], key=lambda m: int(m["channel"]))
        for lo, hi in zip(ms[:-1], ms[1:]):
            want_db = 20 * np.log10(AMPLITUDES[int(hi["channel"])] / AMPLITUDES[int(lo["channel"])])
            assert abs(10 * np.log10(float(hi["signal"]["power"]) / float(lo["signal"]["power"])) - want_db) < 0.3
    host = LongUniq(W).push_heard(prec, rows, signal=psig)
    want = hr.HeardRef(W).push_heard(wrec, wrec["t"], rows, wsig)
    for got in (host, (rec, copies, first, members)):
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[2])
        assert np.array_equal(got[2], want[3]) and got[3].tobytes() == want[4].tobytes()
    urec, ucopies = rig.off.drain_long_frames_unique()      # the twin's unique drain is unchanged
    assert urec.tobytes() == rec.tobytes() and np.array_equal(ucopies, copies)
    assert chain_state(rig.on) == chain_state(rig.off)


# ---- 10. a node of two shards ----------------------------------------------------------------------------------------------
def test_a_node_of_two_shards_equals_one_batch():
    from gnuais_amd import ReceiverBatch, ReceiverNode
    x, W = heard_input(), 64
    b = ReceiverBatch(3, max_len=8192)
    nd = ReceiverNode(3, devices=[0, 0], max_len=8192)
    for q in (b, nd):
        q.frame_times(True)
        q.frame_signal(True)
        q.long_frames(True)
        q.long_frame_signal(True)
        q.long_unique(W)
    half = 9 * 1280
    for lo, hi in ((0, half), (half, len(x))):
        for a in range(lo, hi, 8192):
            e = min(a + 8192, hi)
            b.run_iq(dev(x[a:e]), sync=False)
            nd.run_iq_host(x[a:e])
        nd.sync()
        if lo == 0:                                         # the drain with records
            want, got = b.drain_long_frames_signal(), nd.drain_long_frames_signal()
            assert len(want[0]) >= 3 and np.all(want[1]["blocks"] > 0)
        else:                                               # the heard drain, through the host object with records
            want, got = b.drain_long_frames_heard(), nd.drain_long_frames_heard()
            assert len(want[3]) >= 3 and np.all(want[3]["signal"]["blocks"] > 0)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
    nd.close()


# ---- 11. the state table -------------------------------------------------------------------------------------------------
def test_refusals_their_messages_and_the_info_words():
    from gnuais_amd import ReceiverBatch

    def refused(call, text):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE and text in str(e.value), str(e.value)

    b = ReceiverBatch(4, max_len=4000)
    assert b.info("long_frame_signal") == 0 and b.info("occupancy_lag") == 2762
    refused(lambda: b.long_frame_signal(True), "gnuais_batch_long_frames")
    refused(lambda: b.long_frame_signal(False), "gnuais_batch_long_frames")
    b.long_frames(True)
    refused(lambda: b.long_frame_signal(True), "gnuais_batch_frame_signal")
    refused(b.drain_long_frames_signal, "gnuais_batch_long_frame_signal")
    b.frame_times(True)
    b.frame_signal(True)
    b.occupancy(64, 16)
    refused(lambda: b.long_frame_signal(True), "gnuais_batch_occupancy")
    assert b.info("occupancy_lag") == 2762
    b.occupancy(0)
    b.long_frame_signal(True)
    assert b.info("long_frame_signal") == 1 and b.info("occupancy_lag") == 5562
    refused(lambda: b.frame_signal(False), "gnuais_batch_long_frame_signal")
    assert len(b.drain_long_frames_signal()[0]) == 0
    b.occupancy(64, 16)
    refused(lambda: b.long_frame_signal(False), "gnuais_batch_occupancy")
    refused(lambda: b.long_frame_signal(True), "gnuais_batch_occupancy")
    assert b.info("occupancy_lag") == 5562
    b.occupancy(0)
    b.long_frames(False)                                    # switches the feature off, as it does the long repair
    assert b.info("long_frame_signal") == 0 and b.info("long_frames") == 0 and b.info("frame_signal") == 1
    b.long_frames(True)
    assert b.info("long_frame_signal") == 0
    b.long_frame_signal(True)
    b.long_frame_signal(False)
    assert b.info("long_frame_signal") == 0 and b.info("occupancy_lag") == 2762
    b.frame_signal(False)                                   # allowed again; the larger ring goes with it
    refused(lambda: b.long_frame_signal(True), "gnuais_batch_frame_signal")


def test_feature_off_is_a_batch_that_never_enabled_it():
    """a batch that switched the feature on and off again (and frame_signal anew) against one that never did: long
    records, short records with their signal, occupancy and chain state are the same"""
    from gnuais_amd import ReceiverBatch
    x = lsr.ls9()

    def make(was):
        b = ReceiverBatch(2, max_len=8192)
        b.frame_times(True)
        b.frame_signal(True)
        b.long_frames(True)
        if was:
            b.long_frame_signal(True)
            b.run_iq(dev(x[:3000]))
            b.long_frame_signal(False)
            b.long_frames(False)
            b.long_frames(True)
            b.frame_signal(False)
            b.frame_signal(True)
            b.reset()
        b.occupancy(64, 16)
        return b

    never, was = make(False), make(True)
    for a in range(0, lsr.LS9_ROWS, 8192):
        d = dev(x[a:a + 8192])
        never.run_iq(d, sync=False)
        was.run_iq(d, sync=False)
    assert never.info("occupancy_lag") == was.info("occupancy_lag") == 2762
    assert never.drain_long_frames().tobytes() == was.drain_long_frames().tobytes()
    for g, w in zip(never.drain_frames_signal(), was.drain_frames_signal()):
        assert g.tobytes() == w.tobytes()
    for g, w in zip(never.drain_occupancy(), was.drain_occupancy()):
        assert g.tobytes() == w.tobytes() and len(g) == 14
    assert chain_state(never) == chain_state(was)


# ---- 12. calls in flight -------------------------------------------------------------------------------------------------
def test_calls_in_flight_nbuf_2_k3_on_a_stream_of_its_own(monkeypatch):
    """in the manner of tests/test_tail_pipelined_gpu.py: every call queued behind a blocker with nothing that synchronises
    until the last is queued; the long repair and the occupancy on as well, so the order chain cover, D', long repair, long
    signal and cover, finalisers is the one in flight"""
    import torch
    from test_tail_pipelined_gpu import blocker
    monkeypatch.setenv("GNUAIS_K3_SAME", "0")
    x = lsr.ls9()
    xd = dev(x)
    rig = Rig(2, 5000, repair=True, nbuf=2)
    rig.on.occupancy(64, 16)
    rig.on.run_iq(xd[:64])                                  # everything loaded that a first use loads
    rig.on.reset()
    blocker()
    torch.cuda.synchronize()
    calls = lsr.ragged(lsr.LS9_ROWS)
    for i, (a, e) in enumerate(calls):
        if i == 0:
            ev = blocker()
        rig.on.run_iq(xd[a:e], sync=False)
        if i == 0:
            assert not ev.query(), "the device began before a call was queued"
    want = lsr.ls9_restated()
    rec, sig = rig.on.drain_long_frames_signal()
    assert rec.tobytes() == want["long"].tobytes() and sig.tobytes() == want["long_sig"].tobytes()
    occ_check(rig.on, lsr.ls9_epochs(True), tap=False)      # (469 blocks of code ring: the first epochs' words are gone)
    fr, t, s = rig.on.drain_frames_signal()
    assert fr.tobytes() == want["short"].tobytes() and np.array_equal(t, want["short_t"]) and s.tobytes() == want["short_sig"].tobytes()
    for a, e in calls:                                      # the twin, unhurried
        rig.off.run_iq(xd[a:e])
    assert rig.off.drain_long_frames().tobytes() == rec.tobytes()
    for g, w in zip(rig.off.drain_frames_signal(), (fr, t, s)):
        assert g.tobytes() == w.tobytes()
    assert chain_state(rig.on) == chain_state(rig.off) and np.array_equal(counters3(rig.on), counters3(rig.off))


# ---- 13. scripts/decode_file.py ---------------------------------------------------------------------------------------------
def test_decode_file_long_signal_prints_the_levels_the_drain_gives(tmp_path):
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import signal_dbfs, signal_hz
    x = heard_input()
    path = str(tmp_path / "capture.s16")
    x.tofile(path)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), path, "--raw", "6", "--iq",
                                     "--call", "8192", "--long", *a], check=True, capture_output=True, timeout=300)
    b = ReceiverBatch(3, max_len=8192)
    b.frame_times(True)
    b.frame_signal(True)
    b.long_frames(True)
    b.long_frame_signal(True)
    for a in range(0, len(x), 8192):
        b.run_iq(dev(x[a:a + 8192]), sync=False)
    rec, sig = b.drain_long_frames_signal()
    assert len(rec) == 8 and np.all(sig["blocks"] > 0)
    err = run("--signal").stderr.decode()
    for r, s in zip(rec, sig):
        line = (f"  signal: receiver {int(r['channel'])}, row {int(r['t'])}, {signal_dbfs(s['power']):.1f} dBFS, "
                f"{signal_hz(s['ferr'], 48000):+.0f} Hz\n")
        assert line in err, line
    out = run("--unique", "64", "--heard").stdout.decode()
    heard = [l for l in out.splitlines() if l.startswith("  heard: ") and "dBFS" in l]
    assert len(heard) == 3
    for r, s in zip(rec, sig):
        assert any(f" {signal_dbfs(s['power']):.1f}dBFS {signal_hz(s['ferr'], 48000):+.0f}Hz" in l for l in heard)
