"""The channel load per receiver on the device (gnuais_batch_occupancy, occupancy.hip): every drained record, its first
block and the blocks tap equal tests/occupancy_ref.py's EXACTLY.  The restatement works from the same int16 input and
from the device's own drained frames and times (those are checked against their own restatements elsewhere), over channel
counts on both sides of a finaliser workgroup, ragged calls that take the rings round more than twice, one tail that
makes several epochs final, the codes at both ends, a late switch-on, the AFC, the 192 kHz table, wideband input at an
integer and a rational ratio, the repair, audio calls and decode_bits in between, a reset, stream changes, epochs lost
undrained, a node; the refusals; and the feature off."""
import numpy as np
import pytest

import chan_ref
import iq_ref
import occupancy_ref as orf
import resample_ref as rr
from gnuais_amd import params, synth
from test_iq_gpu import dev, frames_state

pytestmark = pytest.mark.gpu
E, MAX_LEN, TOTAL = 64, 2048, 40000
RAGGED = [1, 63, 64, 65, 777, 2048, 2047, 130]


def calls_of(total, pattern=RAGGED):
    out, pos, i = [], 0, 0
    while pos < total:
        out.append(min(pattern[i % len(pattern)], total - pos))
        pos += out[-1]
        i += 1
    return out


BASE = {}


def iq_input(n_ch, total, seed=3, sps=5, sigma=800.0, amplitude=10000.0, occupancy=0.6):
    """n_ch channels of gated bursts over noise: eight generated streams, each channel one of them turned by its own
    number of rows (computed once per shape and shared)"""
    base = BASE.setdefault((total, seed, sps, sigma, amplitude, occupancy), {})
    for c in range(min(n_ch, 8)):
        if c not in base:
            base[c] = synth.make_iq_stream(total, seed=seed, channel=c, sps=sps, amplitude=amplitude, sigma=sigma,
                                           occupancy=occupancy, gated=True, rate_hz=9600 * sps)[0]
    return np.stack([np.roll(base[c % 8], 997 * (c // 8), axis=0) for c in range(n_ch)], axis=1)


class Pair:
    """a batch (or a node) with the feature on and the restatement, fed the same calls"""

    def __init__(self, b, n_ch, margin=16, pllinc=0x10000 // 5, n_taps=36, W=0, rows=0, E=E):
        self.b, self.n_ch, self.E, self.n, self.seen = b, n_ch, E, rows, 0
        self.ref = orf.OccupancyRef(n_ch, E, margin, pllinc, n_taps, W)
        b.occupancy(E, margin)

    def iq(self, seg, run=None):
        """an I/Q-type call of the rows seg [len][n_ch][2] (run: how the batch takes them, if not run_iq on the device)"""
        if run is None:
            self.b.run_iq(dev(seg), sync=False)
        else:
            run()
        self.ref.run_iq(self.n, seg)
        self.n += len(seg)

    def audio(self, a):
        self.b.run(dev(a), sync=False)
        self.ref.run_audio(self.n, len(a))
        self.n += len(a)

    def check(self, tap=True):
        """the frames so far into the restatement, then one drain against it: first blocks, records, tap words"""
        fr, t, _ = self.b.drain_frames_signal()
        self.ref.add_frames(fr, t)
        first, rec = self.b.drain_occupancy()
        want = self.ref.epochs()[self.seen:]
        assert first.tolist() == [w[0] for w in want], (first, [w[0] for w in want])
        assert rec.dtype == orf.OCCUPANCY_DTYPE and rec.shape == (len(want), self.n_ch)
        b0 = -(-self.ref.runs[-1]["v0"] // 64) if self.ref.runs else 0
        for k, (f0, wrec, words) in enumerate(want):
            assert rec[k].tobytes() == wrec.tobytes(), (f0, np.argwhere(rec[k] != wrec)[:5], rec[k][:3], wrec[:3])
            if tap and f0 >= b0:                             # an epoch of the current run: the ring holds it
                got = self.b.occupancy_blocks(f0, self.E)
                assert np.array_equal(got, words), (f0, np.argwhere(got != words)[:5])
        self.seen += len(want)
        return len(want), rec, fr


def new_batch(n_ch, max_len=MAX_LEN, **kw):
    from gnuais_amd import ReceiverBatch
    b = ReceiverBatch(n_ch, max_len=max_len, **kw)
    b.frame_times(True)
    b.frame_signal(True)
    return b


@pytest.mark.parametrize("n_ch", [1, 3, 65, 130])
def test_records_and_tap_ragged_calls_round_the_rings(n_ch):
    """40 000 rows in calls of 1 to 2048: the code and cover rings (270 blocks) go round more than twice; 65 and 130
    channels: a second and a third finaliser workgroup, partly empty"""
    x = iq_input(n_ch, TOTAL)
    b = new_batch(n_ch)
    assert b.info("occupancy") == 0
    p = Pair(b, n_ch)
    assert b.info("occupancy") == E
    pos, n_ep, busy, covered = 0, 0, 0, 0
    for i, n in enumerate(calls_of(TOTAL)):
        p.iq(x[pos:pos + n])
        pos += n
        if i % 8 == 7:
            k, rec, _ = p.check()
            n_ep += k
            busy += int(rec["busy"].sum())
            covered += int(rec["covered"].sum())
    n_ep += p.check()[0]
    assert n_ep == (TOTAL - orf.lag(0x10000 // 5)) // (64 * E) == 9 and b.occupancy_lost() == 0
    assert busy > 9 * E * n_ch * 0.3 and 0.5 * busy < covered <= busy


def test_one_tail_makes_several_epochs_final():
    n_ch = 5
    x = iq_input(n_ch, 13000)
    b = new_batch(n_ch, max_len=10000)
    p = Pair(b, n_ch)
    p.iq(x[:3000])
    assert p.check()[0] == 0
    p.iq(x[3000:])
    assert p.check()[0] == 2


@pytest.mark.parametrize("margin", [255, 1])
def test_codes_at_both_ends_and_ties_at_the_rank(margin):
    """whole blocks of (0, 0), (-32768, -32768) and (32767, -32768): codes 0 and 280; a channel of zeros throughout (every
    code ties at the rank) and one of full scale throughout; margin 255: nothing is busy anywhere"""
    n_ch, total = 4, 4 * 64 * E + orf.lag(0x10000 // 5) + 100
    x = np.random.default_rng(5).integers(-300, 300, (total, n_ch, 2)).astype(np.int16)
    for lo in range(0, total - 640, 1024):
        x[lo + 64:lo + 192, 0] = -32768
        x[lo + 256:lo + 384, 0, 0], x[lo + 256:lo + 384, 0, 1] = 32767, -32768
        x[lo + 448:lo + 576, 0] = 0
    x[:, 1] = 0
    x[:, 2] = -32768
    b = new_batch(n_ch)
    p = Pair(b, n_ch, margin=margin)
    recs = []
    for lo in range(0, total, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN])
        recs.append(p.check()[1])
    rec = np.concatenate(recs)
    assert len(rec) == 4 and np.all(rec["floor"][:, 1] == 0) and np.all(rec["floor"][:, 2] == 280)
    assert np.all(rec["busy"][:, 1:3] == 0)
    if margin == 255:
        assert np.all(rec["busy"] == 0) and np.all(rec["bursts"] == 0)                # no code reaches a floor + 255
    else:
        assert np.all(rec["busy"][:, 0] >= 16) and np.all(rec["busy"][:, 3] > 0)


def test_switch_on_mid_stream_v0_inside_a_block():
    from gnuais_amd import ReceiverBatch
    n_ch = 6
    x = iq_input(n_ch, 20000)
    b = ReceiverBatch(n_ch, max_len=MAX_LEN)
    b.frame_times(True)
    b.run_iq(dev(x[:1000]), sync=False)
    b.frame_signal(True)
    b.run_iq(dev(x[1000:1501]), sync=False)                  # the signal ring's run starts at 1000, the epochs' at 1501
    b.drain_frames()
    p = Pair(b, n_ch, rows=1501)
    n_ep = 0
    for lo in range(1501, 20000, 1999):
        p.iq(x[lo:lo + 1999])
        n_ep += p.check()[0]
    assert n_ep == 3 and p.ref.epochs()[0][0] == 24


def test_with_the_afc_window_1024():
    from gnuais_amd.lib import E_STATE, GnuaisError
    n_ch, W = 7, 1024
    x = iq_input(n_ch, 24000)
    b = new_batch(n_ch)
    b.afc(W)
    p = Pair(b, n_ch, W=W)
    with pytest.raises(GnuaisError) as e:
        b.afc(2048)                                         # the rings are sized for the window in use
    assert e.value.code == E_STATE
    n_ep = covered = 0
    for lo in range(0, 24000, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN])
        k, rec, _ = p.check()
        n_ep += k
        covered += int(rec["covered"].sum())
    assert n_ep == (24000 - orf.lag(0x10000 // 5, 36, W)) // (64 * E) == 5 and covered > 100


def test_the_192k_table_short_stream():
    n_ch, sps = 3, 20
    total = 6 * synth.SLOT_BITS * sps
    x = iq_input(n_ch, total, seed=7, sps=sps)
    calls = [1, 777, 2049, 12000]
    calls.append(total - sum(calls))
    b = new_batch(n_ch, max_len=max(calls), taps=params.taps_192k(), pllinc=params.PLLINC_192K)
    p = Pair(b, n_ch, pllinc=params.PLLINC_192K, n_taps=len(params.taps_192k()))
    pos, n_ep, covered = 0, 0, 0
    for n in calls:
        p.iq(x[pos:pos + n])
        pos += n
        k, rec, _ = p.check()
        n_ep += k
        covered += int(rec["covered"].sum())
    assert n_ep == (total - orf.lag(params.PLLINC_192K, len(params.taps_192k()))) // (64 * E) >= 4 and covered > 50


def test_wideband_integer_ratio():
    """the channeliser at D = 6, K = 2: x[n] is its output pair"""
    M, D, offs = 5, 6, (-25000, 25000)
    N, n = M * len(offs), 12 * 1280 * D
    x = np.stack([synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=s, amplitude=1500.0, sigma=225.0,
                                             occupancy=0.8, gated=True)[0] for s in range(M)], axis=1)
    b = new_batch(N)
    b.channeliser(D, 48000 * D, offs)
    p, ch = Pair(b, N), chan_ref.Channeliser(M, D, 48000 * D, offs)
    n_ep = covered = 0
    for lo in range(0, n, D * 1500):
        seg = x[lo:lo + D * 1500]
        p.iq(ch.run(seg), run=lambda: b.run_wideband(dev(seg), sync=False))
        k, rec, _ = p.check()
        n_ep += k
        covered += int(rec["covered"].sum())
    assert n_ep == 3 and covered > 100


def test_wideband_resampler_3_64():
    up, down, M, offs = 3, 64, 2, [-25000, 25000]
    N, rate = M * len(offs), 48000 * down // up
    n = 12 * 1280 * down // up
    x = np.stack([synth.make_resampled_wideband_stream(n, up, down, (-25000, 25000), seed=5, stream=s, sigma=300.0,
                                                       occupancy=0.7, gated=True)[0] for s in range(M)], axis=1)
    periods = n // down
    cuts = [0, 1, periods // 8, periods // 8 + 1, periods // 3, periods]
    rows = max(b - a for a, b in zip(cuts[:-1], cuts[1:])) * up
    b = new_batch(N, max_len=rows)
    b.resampler(up, down, rate, offs)
    p, r = Pair(b, N), rr.Resampler(M, up, down, rate, offs)
    n_ep = covered = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = x[a * down:e * down]
        p.iq(r.run(seg), run=lambda: b.run_wideband(dev(seg), sync=False))
        k, rec, _ = p.check()
        n_ep += k
        covered += int(rec["covered"].sum())
    assert n_ep == 3 and covered > 30


def test_repaired_frames_cover_like_any_frame():
    n_ch, total = 12, 20 * 1280
    x = iq_input(n_ch, total, seed=20, sigma=700.0, amplitude=3000.0, occupancy=0.8)
    b = new_batch(n_ch)
    b.repair(True)
    p = Pair(b, n_ch)
    n_ep, n_rep = 0, 0
    for lo in range(0, total, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN])
        k, _, fr = p.check()
        n_ep += k
        n_rep += int(((fr["flags"] & 0x40) != 0).sum())
    assert n_ep == 5 and n_rep >= 3


def test_an_audio_call_and_decode_bits_between_iq_calls():
    """decode_bits between two I/Q-type calls leaves the run alone (its frames have no time and cover nothing); an
    audio-type call ends it: the open epoch is dropped, the numbering starts again at the next I/Q-type call's first
    whole block, and the tap no longer serves the blocks of the run before"""
    from gnuais_amd.lib import E_ARG, GnuaisError
    from oracle_lib import Oracle
    n_ch = 6
    x = iq_input(n_ch, 30000)
    audio = iq_ref.discriminate(x, None)[0]
    b = new_batch(n_ch, max_len=4000)
    p = Pair(b, n_ch)
    cuts = [0, 4000, 8000, 11001, 11702, 15000, 19000, 23000, 27000, 30000]
    kinds = ["iq", "iq", "iq", "audio", "iq", "iq", "iq", "iq", "iq"]
    firsts = []
    for i, (lo, hi, kind) in enumerate(zip(cuts[:-1], cuts[1:], kinds)):
        if i == 1:
            b.decode_bits(Oracle(n_ch).run(audio[:3 * 1280], want_bits=True)["bits"])
        if kind == "iq":
            p.iq(x[lo:hi])
        else:
            p.audio(audio[lo:hi])
        k = p.check()[0]
        firsts += [e[0] for e in p.ref.epochs()[p.seen - k:p.seen]]
    assert firsts == [0, 64, 183, 247, 311]                # 11001 rows: two epochs final, the third dropped; 11702 = 64 * 182.8
    with pytest.raises(GnuaisError) as e:
        b.occupancy_blocks(64, 64)                          # of the run before
    assert e.value.code == E_ARG


def test_reset_empties_the_queue_and_starts_at_row_0():
    n_ch = 4
    x = iq_input(n_ch, 16000)
    b = new_batch(n_ch)
    p = Pair(b, n_ch)
    for lo in range(0, 16000, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN])
    b.sync()
    b.reset()                                               # three final epochs undrained: gone
    first, rec = b.drain_occupancy()
    assert len(first) == 0 and b.occupancy_lost() == 0 and b.info("occupancy") == E and b.info("rows") == 0
    p.ref.reset()
    p.n = p.seen = 0
    n_ep = 0
    for lo in range(300, 16000, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN])
        n_ep += p.check()[0]
    assert n_ep == 3


def test_a_stream_change_between_calls():
    """every call on another stream and nothing synchronised by the caller"""
    import torch
    n_ch, rows, n_calls = 64, 2000, 12
    x = iq_input(n_ch, rows * n_calls)
    xd = dev(x)
    b = new_batch(n_ch)
    p = Pair(b, n_ch)
    streams = [torch.cuda.Stream() for _ in range(3)]
    for i in range(n_calls):
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        seg = xd[i * rows:(i + 1) * rows]
        with torch.cuda.stream(st):
            p.iq(x[i * rows:(i + 1) * rows], run=lambda: b.run_iq(seg, sync=False))
    assert p.check(tap=False)[0] == 5                       # the first epochs' tap words are a ring round behind
    torch.cuda.synchronize()


def test_seventy_epochs_undrained_six_are_lost():
    n_ch = 3
    total = 70 * 64 * E + orf.lag(0x10000 // 5) + 1
    x = iq_input(n_ch, total, occupancy=0.5)
    xd = dev(x)
    b = new_batch(n_ch)
    p = Pair(b, n_ch)
    for lo in range(0, total, MAX_LEN):
        p.iq(x[lo:lo + MAX_LEN], run=lambda: b.run_iq(xd[lo:lo + MAX_LEN], sync=False))
        if lo % (8 * MAX_LEN) == 0:
            fr, t, _ = b.drain_frames_signal()              # the frames only: the epochs stay queued
            p.ref.add_frames(fr, t)
    assert b.occupancy_lost() == 6
    p.seen = 6
    assert p.check(tap=False)[0] == 64 and b.occupancy_lost() == 6
    assert len(b.drain_occupancy()[0]) == 0


def test_a_node_of_two_shards_equals_one_batch():
    from gnuais_amd import ReceiverNode
    n_ch, total, rows = 7, 16000, 4000
    x = iq_input(n_ch, total, seed=12)
    nd = ReceiverNode(n_ch, devices=[0, 0], max_len=rows)
    nd.frame_times(True)
    nd.frame_signal(True)
    b = new_batch(n_ch, max_len=rows)
    pn, pb = Pair(nd, n_ch), Pair(b, n_ch)
    for lo in range(0, total, rows):
        pn.iq(x[lo:lo + rows], run=lambda: nd.run_iq_host(x[lo:lo + rows]))
        pb.iq(x[lo:lo + rows])
    nd.sync()
    fr, t, _ = nd.drain_frames_signal()
    pn.ref.add_frames(fr, t)
    first, rec = nd.drain_occupancy()
    want = pn.ref.epochs()
    assert first.tolist() == [w[0] for w in want] == [0, 64, 128] and all(rec[k].tobytes() == want[k][1].tobytes() for k in range(3))
    fr_b, t_b, _ = b.drain_frames_signal()
    first_b, rec_b = b.drain_occupancy()
    assert np.array_equal(first, first_b) and rec.tobytes() == rec_b.tobytes() and fr.tobytes() == fr_b.tobytes()
    nd.close()


def test_refusals():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_ARG, E_STATE, GnuaisError

    def refused(call, code=E_STATE):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == code

    n_ch = 8
    b = ReceiverBatch(n_ch, max_len=4000)
    refused(lambda: b.occupancy(64, 16))                    # the signal ring is off
    refused(b.drain_occupancy)
    refused(lambda: b.occupancy_blocks(0, 1))
    b.frame_times(True)
    refused(lambda: b.occupancy(64, 16))
    b.frame_signal(True)
    for E_bad, m_bad in ((63, 16), (4097, 16), (-1, 16), (64, 0), (64, 256)):
        refused(lambda: b.occupancy(E_bad, m_bad), E_ARG)
    b.occupancy(64, 16)
    for call in (lambda: b.frame_signal(False), lambda: b.set_option("nbuf", 4), b.stream_nmea,
                 lambda: b.set_option("streaming", 1), lambda: b.afc(128)):
        refused(call)
    refused(lambda: b.occupancy_blocks(0, 1), E_ARG)        # nothing final yet
    assert b.occupancy_lost() == 0 and len(b.drain_occupancy()[0]) == 0
    b.set_option("nbuf", 2)                                 # below the depth it was sized at
    b.occupancy(0)
    assert b.info("occupancy") == 0
    b.frame_signal(False)
    b.set_option("nbuf", 4)
    s = ReceiverBatch(n_ch, max_len=4000)                   # a streaming batch
    s.stream_nmea()
    refused(lambda: s.occupancy(64, 16))


def test_feature_off_is_a_batch_that_never_enabled_it():
    """a batch that switched the feature on, ran with it and switched it off again delivers the frames, times and signal
    records of one that never did"""
    n_ch, total = 29, 16 * 1280
    x = iq_input(n_ch, total)
    calls = [1020, 1, 2048, 333, 2000]
    calls += calls_of(total - sum(calls), [2048])
    never, was = new_batch(n_ch), new_batch(n_ch)
    was.occupancy(64, 16)
    was.run_iq(dev(x[:3000][:MAX_LEN]))
    was.occupancy(0)
    was.reset()
    pos = 0
    for n in calls:
        never.run_iq(dev(x[pos:pos + n]), sync=False)
        was.run_iq(dev(x[pos:pos + n]), sync=False)
        pos += n
    out = []
    for b in (never, was):
        b.sync()
        fr, t, sig = b.drain_frames_signal()
        out.append((fr.tobytes(), t.tobytes(), sig.tobytes()))
        assert len(fr) > 100 and (sig["blocks"] > 0).sum() > 100
    assert out[0] == out[1]
    assert frames_state(never)[1:] == frames_state(was)[1:]
