"""The frames' signal power and carrier error on the device (gnuais_batch_frame_signal, frame_signal.hip): the ring's block
sums and every drained record equal tests/frame_signal_ref.py's EXACTLY, with the frames and their times, over lane
widths, ragged calls that wrap the ring, the values at the edge of 32 bits, I/Q and wideband input at an integer and a
rational ratio, the AFC, the host forms, a node, the repair, a reset, a late switch-on, audio calls and decode_bits in
between, stream changes, both PLL forms and the 192 kHz table; the refusals; and the feature off."""
import numpy as np
import pytest

import afc_ref
import chan_ref
import frame_signal_ref as fsr
import frame_time_ref as ftr
import iq_ref
import resample_ref as rr
from gnuais_amd import params, synth
from test_iq_gpu import dev, frames_state

pytestmark = pytest.mark.gpu
RAGGED = [1, 63, 64, 65, 777, 2048, 2047, 130]


def calls_of(total, pattern=RAGGED):
    out, pos, i = [], 0, 0
    while pos < total:
        out.append(min(pattern[i % len(pattern)], total - pos))
        pos += out[-1]
        i += 1
    return out


def edge_pairs(n_rows, n_ch, seed):
    """random full-range pairs with whole blocks of (-32768, -32768), (32767, -32768) and 0 every 2048 rows: P and r at
    2^31, in every pass round the ring"""
    x = np.random.default_rng(seed).integers(-32768, 32768, (n_rows, n_ch, 2)).astype(np.int16)
    for lo in range(0, n_rows - 640, 2048):
        x[lo + 64:lo + 192] = -32768
        x[lo + 256:lo + 384, :, 0], x[lo + 256:lo + 384, :, 1] = 32767, -32768
        x[lo + 448:lo + 576] = 0
    return x


@pytest.mark.parametrize("n_ch,offset", [(1, False), (3, False), (65, False), (130, False), (64, True)])
def test_signal_blocks_equal_the_restatement_ragged_calls_round_the_ring(n_ch, offset):
    """channel counts that reach every lane width (130: two per lane, 64: four; with the pointer 4 bytes in: one), 40 x
    1280 rows in calls of at most 2048, so the ring (nbuf + 2 calls and the longest span) is gone round more than twice"""
    import torch
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_ARG, GnuaisError
    total = 40 * 1280
    x = edge_pairs(total, n_ch, 200 + n_ch)
    if offset:
        flat = torch.cat([torch.zeros(2, dtype=torch.int16), torch.from_numpy(x.reshape(-1))]).cuda()
        xd = flat[2:].view(total, n_ch, 2)
        assert xd.data_ptr() % 8 == 4
    else:
        xd = dev(x)
    b = ReceiverBatch(n_ch, max_len=2048)
    b.frame_times(True)
    assert b.info("frame_signal") == 0
    b.frame_signal(True)
    assert b.info("frame_signal") == 1
    ref = fsr.BlockSums(n_ch)
    pos = 0
    for n in calls_of(total):
        b.run_iq(xd[pos:pos + n], sync=False)
        ref.feed(pos, x[pos:pos + n])
        j0, j1 = pos // 64, -(-(pos + n) // 64)
        got = b.signal_blocks(j0, j1 - j0)
        assert np.array_equal(got, ref.blocks(j0, j1 - j0)), (pos, n, np.argwhere(got != ref.blocks(j0, j1 - j0))[:4])
        pos += n
    assert ref.blk[:, :, 0].max() == 64 << 31 and ref.blk[:, :, 1].max() == 64 << 31      # beyond int32, exact
    end = total // 64
    held = b.signal_blocks(end - 300, 300)
    assert np.array_equal(held, ref.blocks(end - 300, 300))
    for j0, count in ((0, 1), (end - 5000 // 64 - 300, 1), (end, 1), (end - 1, 2)):      # replaced long ago; not yet written
        with pytest.raises(GnuaisError) as e:
            b.signal_blocks(j0, count)
        assert e.value.code == E_ARG


def check_drain(b, ref):
    """one drain against the restatement: the same frames in the same order, the same times, the same records"""
    fr, t, sig = b.drain_frames_signal()
    wf, wt, ws = ref.drain()
    assert fr.tobytes() == wf.tobytes(), (len(fr), len(wf))
    assert np.array_equal(t, wt)
    assert sig.dtype == fsr.SIGNAL_DTYPE and sig.tobytes() == ws.tobytes(), np.argwhere(sig != ws)[:5]
    return fr, t, sig


def iq_input(n_ch, total, offset_hz=0.0, seed=3, sps=5, sigma=800.0, amplitude=10000.0):
    return np.stack([synth.make_iq_stream(total, seed=seed, channel=c, sps=sps, amplitude=amplitude, sigma=sigma,
                                          occupancy=0.8, gated=True, offset_hz=offset_hz, rate_hz=9600 * sps)[0]
                     for c in range(n_ch)], axis=1)


class Front:
    """the stages in front of the chain, restated: I/Q -> the audio the chain takes"""

    def __init__(self, n_ch, W):
        self.afc, self.carry = (afc_ref.Afc(n_ch, W) if W else None), None

    def audio(self, iq):
        if self.afc:
            return self.afc.apply(iq)
        a, self.carry = iq_ref.discriminate(iq, self.carry)
        return a

    def reset(self):
        self.carry = None
        if self.afc:
            self.afc.reset()


@pytest.mark.parametrize("W,variant", [(0, 7), (0, 8), (1024, 7)])
def test_records_run_iq_device_and_host_forms_both_pll_forms(W, variant):
    """run_iq on device input (queued, a drain in the middle) and run_iq_host on the same calls; with the AFC at a 3 kHz
    carrier error the records still measure the raw I/Q: ferr is near 3 kHz"""
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import signal_dbfs, signal_hz
    n_ch, total = 29, 16 * 1280
    x = iq_input(n_ch, total, 3000.0 if W else 0.0)
    calls = [1020, 1, 4096, 333, 7000]
    calls.append(total - sum(calls))
    d, h = ReceiverBatch(n_ch, max_len=max(calls)), ReceiverBatch(n_ch, max_len=max(calls))
    ref, front = fsr.FrameSignalRef(n_ch, afc_window=W), Front(n_ch, W)
    ref_h = fsr.FrameSignalRef(n_ch, afc_window=W)           # the host form is drained once, at the end
    for b in (d, h):
        b.set_option("pll_variant", variant)
        if W:
            b.afc(W)
        b.frame_times(True)
        b.frame_signal(True)
    ref.switch_on()
    ref_h.switch_on()
    pos, sigs = 0, []
    for i, n in enumerate(calls):
        seg = x[pos:pos + n]
        pos += n
        d.run_iq(dev(seg), sync=False)
        h.run_iq(seg)
        audio = front.audio(seg)
        ref.run_iq(seg, audio)
        ref_h.run_iq(seg, audio)
        if i == 2:
            sigs.append(check_drain(d, ref)[2])
    sigs.append(check_drain(d, ref)[2])
    sig = np.concatenate(sigs)
    assert len(sig) > 100 and (sig["blocks"] == 14).sum() > 100
    hf, ht, hs = check_drain(h, ref_h)
    ok = sig[sig["blocks"] > 0]
    assert len(hf) == len(sig) and np.array_equal(np.sort(hs, order=["power", "ferr", "blocks"]), np.sort(sig, order=["power", "ferr", "blocks"]))
    assert abs(signal_hz(ok["ferr"], 48000).mean() - (3000.0 if W else 0.0)) < 100.0
    assert abs(signal_dbfs(ok["power"]).mean() - 10 * np.log10((1e8 + 2 * 800.0 ** 2) / 2 ** 31)) < 0.2


def test_records_run_wideband_integer_ratio():
    """the channeliser at D = 6, K = 2: x[n] is its output pair"""
    from gnuais_amd import ReceiverBatch
    M, D, offs = 5, 6, (-25000, 25000)
    N, n = M * len(offs), 12 * 1280 * D
    x = np.stack([synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=s, amplitude=1500.0, sigma=225.0,
                                             occupancy=0.8, gated=True)[0] for s in range(M)], axis=1)
    calls = [D * 1020, D, D * 4096, D * 333]
    calls.append(n - sum(calls))
    b = ReceiverBatch(N, max_len=max(calls) // D)
    b.channeliser(D, 48000 * D, offs)
    b.frame_times(True)
    b.frame_signal(True)
    ch, ref, front = chan_ref.Channeliser(M, D, 48000 * D, offs), fsr.FrameSignalRef(N), Front(N, 0)
    ref.switch_on()
    pos = 0
    for c in calls:
        b.run_wideband(dev(x[pos:pos + c]), sync=False)
        iq = ch.run(x[pos:pos + c])
        ref.run_iq(iq, front.audio(iq))
        pos += c
    fr, _, sig = check_drain(b, ref)
    assert len(fr) > 60 and (sig["blocks"] == 14).sum() > 60


def test_records_resampler_3_64_device_host_and_a_node_of_two_shards():
    """the rational wide stage at 3/64 on device input, on host input and on a node of two shards"""
    from gnuais_amd import ReceiverBatch, ReceiverNode
    up, down, M, offs = 3, 64, 2, [-25000, 25000]
    N, rate = M * len(offs), 48000 * down // up
    n = 12 * 1280 * down // up
    x = np.stack([synth.make_resampled_wideband_stream(n, up, down, (-25000, 25000), seed=5, stream=s, sigma=300.0,
                                                       occupancy=0.7, gated=True)[0] for s in range(M)], axis=1)
    periods = n // down
    cuts = [0, 1, periods // 8, periods // 8 + 1, periods // 3, periods]
    rows = max(b - a for a, b in zip(cuts[:-1], cuts[1:])) * up
    d, h = ReceiverBatch(N, max_len=rows), ReceiverBatch(N, max_len=rows)
    nd = ReceiverNode(N, devices=[0, 0], max_len=rows)
    for b in (d, h, nd):
        b.resampler(up, down, rate, offs)
        b.frame_times(True)
        b.frame_signal(True)
    r, ref, front = rr.Resampler(M, up, down, rate, offs), fsr.FrameSignalRef(N), Front(N, 0)
    ref.switch_on()
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = x[a * down:e * down]
        d.run_wideband(dev(seg), sync=False)
        h.run_wideband(seg)
        nd.run_wideband_host(seg)
        iq = r.run(seg)
        ref.run_iq(iq, front.audio(iq))
    nd.sync()
    wf, wt, ws = ref.drain()
    assert len(wf) > 10 and (ws["blocks"] == 14).sum() > 10
    for b in (d, h, nd):
        fr, t, sig = b.drain_frames_signal()
        assert fr.tobytes() == wf.tobytes() and np.array_equal(t, wt) and sig.tobytes() == ws.tobytes()
    nd.close()


def test_records_node_run_iq_host_global_channels():
    from gnuais_amd import ReceiverNode
    n_ch, total, rows = 7, 8 * 1280, 4000
    x = iq_input(n_ch, total, seed=12)
    nd = ReceiverNode(n_ch, devices=[0, 0], max_len=rows)
    nd.frame_times(True)
    nd.frame_signal(True)
    ref, front = fsr.FrameSignalRef(n_ch), Front(n_ch, 0)
    ref.switch_on()
    for lo in range(0, total, rows):
        nd.run_iq_host(x[lo:lo + rows])
        ref.run_iq(x[lo:lo + rows], front.audio(x[lo:lo + rows]))
    nd.sync()
    fr, _, sig = check_drain(nd, ref)
    assert len(fr) > 30 and len(np.unique(fr["channel"])) == n_ch and (sig["blocks"] == 14).sum() > 30
    nd.close()


def test_repaired_frames_carry_a_record():
    """a noisy stream with the repair on: the received frames, their times and records equal the restatement's; every
    repaired frame's record is the restatement's for its time, and measured"""
    from gnuais_amd import ReceiverBatch
    n_ch, total = 12, 20 * 1280
    x = iq_input(n_ch, total, seed=20, sigma=700.0, amplitude=3000.0)
    calls = calls_of(total, [4096, 777, 6000])
    b = ReceiverBatch(n_ch, max_len=max(calls))
    b.repair(True)
    b.frame_times(True)
    b.frame_signal(True)
    ref, front = fsr.FrameSignalRef(n_ch), Front(n_ch, 0)
    ref.switch_on()
    pos = 0
    for n in calls:
        b.run_iq(dev(x[pos:pos + n]), sync=False)
        ref.run_iq(x[pos:pos + n], front.audio(x[pos:pos + n]))
        pos += n
    fr, t, sig = b.drain_frames_signal()
    rep = (fr["flags"] & 0x40) != 0
    assert rep.sum() >= 5 and rep.sum() == b.repaired().sum()
    assert sig[rep].tobytes() == ref.records_for(fr[rep], t[rep]).tobytes() and np.all(sig[rep]["blocks"] > 0)
    wf, wt, ws = ref.drain()
    assert fr[~rep].tobytes() == wf.tobytes() and np.array_equal(t[~rep], wt) and sig[~rep].tobytes() == ws.tobytes()
    assert len(wf) > 50


def test_reset_late_switch_on_audio_calls_and_decode_bits_in_between():
    """frames appended before the switch give (0, 0, 0); an audio call between I/Q calls zeroes its own frames and every
    frame whose span reaches behind it; decode_bits gives t = -1 and (0, 0, 0); a reset starts a new run at row 0"""
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    n_ch, total = 6, 24 * 1280
    x = iq_input(n_ch, total, seed=8)
    audio = iq_ref.discriminate(x, None)[0]
    b = ReceiverBatch(n_ch, max_len=8000)
    b.frame_times(True)
    ref, front = fsr.FrameSignalRef(n_ch), Front(n_ch, 0)
    cuts = [0, 5000, 5000 + 6 * 1280 + 300, 13000 + 2 * 1280 + 100, 21000, 27000, total]
    kinds = ["iq", "iq", "audio", "iq", "iq", "iq"]
    n_zero = n_ok = 0
    for i, (lo, hi, kind) in enumerate(zip(cuts[:-1], cuts[1:], kinds)):
        if i == 1:                                           # the first call ran without the feature
            b.frame_signal(True)
            ref.switch_on()
        if i == 4:
            bits = Oracle(n_ch).run(audio[:3 * 1280], want_bits=True)["bits"]
            b.decode_bits(bits)
            ref.decode_bits(bits)
        if kind == "iq":
            b.run_iq(dev(x[lo:hi]), sync=False)
            ref.run_iq(x[lo:hi], front.audio(x[lo:hi]))
        else:                                                # the same rows as audio: the run of I/Q calls breaks here
            b.run(dev(audio[lo:hi]), sync=False)
            ref.run_audio(audio[lo:hi])                      # (the discriminator's own carry stays: the last I/Q call's last pair)
        if i in (1, 3, 5):
            fr, t, sig = check_drain(b, ref)
            n_zero += int((sig["blocks"] == 0).sum())
            n_ok += int((sig["blocks"] > 0).sum())
            if i == 1:
                assert np.all(sig[t < cuts[1]]["blocks"] == 0) and (t < cuts[1]).sum() > 5
            if i == 3:
                assert np.all(sig[(t >= cuts[2]) & (t < cuts[3])]["blocks"] == 0)
            if i == 5:
                assert (t == -1).sum() >= 3 and np.all(sig[t == -1]["blocks"] == 0)
    assert n_zero > 20 and n_ok > 50
    b.reset()
    ref.reset()
    front.reset()
    assert b.info("frame_signal") == 1 and b.info("rows") == 0
    b.run_iq(dev(x[:7000]))
    ref.run_iq(x[:7000], front.audio(x[:7000]))
    fr, t, sig = check_drain(b, ref)
    assert len(fr) > 15 and (sig["blocks"] == 14).sum() > 15


def test_records_with_a_stream_change_between_calls():
    """every call on another stream and nothing synchronised by the caller"""
    import torch
    from gnuais_amd import ReceiverBatch
    n_ch, rows, n_calls = 64, 3000, 7
    x = iq_input(n_ch, rows * n_calls, seed=5)
    xd = dev(x)
    b = ReceiverBatch(n_ch, max_len=rows)
    b.frame_times(True)
    b.frame_signal(True)
    ref, front = fsr.FrameSignalRef(n_ch), Front(n_ch, 0)
    ref.switch_on()
    streams = [torch.cuda.Stream() for _ in range(3)]
    for i in range(n_calls):
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            b.run_iq(xd[i * rows:(i + 1) * rows], sync=False)
        seg = x[i * rows:(i + 1) * rows]
        ref.run_iq(seg, front.audio(seg))
    fr, _, sig = check_drain(b, ref)
    torch.cuda.synchronize()
    assert len(fr) > 64 * 8


def test_records_192k_table_short_stream():
    from gnuais_amd import ReceiverBatch
    n_ch, sps = 3, 20
    total = 6 * synth.SLOT_BITS * sps
    x = iq_input(n_ch, total, seed=7, sps=sps)
    calls = [1, 777, 2049, 12000]
    calls.append(total - sum(calls))
    b = ReceiverBatch(n_ch, taps=params.taps_192k(), pllinc=params.PLLINC_192K, max_len=max(calls))
    b.frame_times(True)
    b.frame_signal(True)
    ref, front = fsr.FrameSignalRef(n_ch, params.taps_192k(), params.PLLINC_192K), Front(n_ch, 0)
    ref.switch_on()
    pos = 0
    for n in calls:
        b.run_iq(dev(x[pos:pos + n]), sync=False)
        ref.run_iq(x[pos:pos + n], front.audio(x[pos:pos + n]))
        pos += n
    fr, _, sig = check_drain(b, ref)
    assert len(fr) >= 8 and (sig["blocks"] == 59).sum() >= 8        # S = 3840 rows: 59 or 60 whole blocks


def test_refusals():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_STATE, GnuaisError

    def refused(call):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE

    n_ch = 8
    b = ReceiverBatch(n_ch, max_len=4000)
    refused(lambda: b.frame_signal(True))                   # frame times are off
    refused(b.drain_frames_signal)
    refused(lambda: b.signal_blocks(0, 1))
    b.frame_times(True)
    b.frame_signal(True)
    for call in (b.stream_nmea, lambda: b.set_option("streaming", 1), lambda: b.frame_times(False),
                 lambda: b.set_option("nbuf", 4)):
        refused(call)
    b.frame_signal(False)
    assert b.info("frame_signal") == 0
    b.set_option("nbuf", 4)
    b.frame_times(False)
    s = ReceiverBatch(n_ch, max_len=4000)                   # a streaming batch
    s.stream_nmea()
    refused(lambda: s.frame_signal(True))
    s.set_option("streaming", 0)
    s.frame_times(True)
    s.frame_signal(True)
    assert s.info("frame_signal") == 1


def test_feature_off_is_a_batch_that_never_enabled_it():
    """drain_frames_timed on a batch that never switched the feature on, and on one that switched it off again, gives
    what it gave before there was a feature: tests/test_frame_times_gpu.py's run_iq input against the times' restatement"""
    from gnuais_amd import ReceiverBatch
    n_ch, total = 29, 16 * 1280
    x = np.stack([synth.make_iq_stream(total, seed=3, channel=c, sigma=800.0, occupancy=0.8, gated=True)[0]
                  for c in range(n_ch)], axis=1)
    calls = [1020, 1, 4096, 333, 7000]
    calls.append(total - sum(calls))
    never, was = ReceiverBatch(n_ch, max_len=max(calls)), ReceiverBatch(n_ch, max_len=max(calls))
    never.frame_times(True)
    was.frame_times(True)
    was.frame_signal(True)
    was.run_iq(dev(x[:3000]))
    was.frame_signal(False)
    was.reset()
    ref, carry = ftr.FrameTimeRef(n_ch), None
    pos = 0
    for n in calls:
        seg = x[pos:pos + n]
        pos += n
        never.run_iq(dev(seg), sync=False)
        was.run_iq(dev(seg), sync=False)
        audio, carry = iq_ref.discriminate(seg, carry)
        ref.run(audio)
    wf, wt = ref.drain()
    for b in (never, was):
        b.sync()
        fr, t = b.drain_frames_timed()
        assert fr.tobytes() == wf.tobytes() and np.array_equal(t, wt) and len(fr) > 100
    assert frames_state(never)[1:] == frames_state(was)[1:]
