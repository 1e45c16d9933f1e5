"""The frames' receive times on the device (gnuais_batch_frame_times, frame_time.hip): the times of every drained frame
equal tests/frame_time_ref.py's EXACTLY and the frames equal the plain drain's / the oracle's, over batch sizes, ragged
calls, both PLL forms, the 192 kHz table, I/Q and wideband input, the AFC, queued and drained-per-call use, stream
changes, the resets, decode_bits, a late switch-on, a node, and one C3-size call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import afc_ref
import chan_ref
import frame_time_ref as ftr
import iq_ref
from gnuais_amd import params, synth
from test_iq_gpu import dev, frames_state
from wide_format_ref import convert, quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RAGGED = [1, 777, 2047, 2048, 2049, 48000]


def tiled(n_ch, total, sps=5, seed=7, n_base=16):
    base, _ = synth.make_base_streams(min(n_ch, n_base), total, seed=seed, sps=sps, occupancy=0.8)
    return synth.tile_channels(base, n_ch)


def check_drain(b, ref):
    """one timed drain against the restatement: the same frames in the same order, the same times; -> (frames, times)"""
    fr, t = b.drain_frames_timed()
    wf, wt = ref.drain()
    assert fr.tobytes() == wf.tobytes(), (len(fr), len(wf))
    assert t.dtype == np.int64 and np.array_equal(t, wt), np.argwhere(t != wt)[:5]
    return fr, t


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("n_ch", [1, 3, 65, 1000])
def test_times_equal_the_restatement_ragged_calls_both_pll_forms(n_ch, variant):
    """a drain after every call, then -- after a reset -- the same calls queued without a sync and drained once"""
    from gnuais_amd import ReceiverBatch
    total = sum(RAGGED)
    x = tiled(n_ch, total)
    xd = dev(x)
    b = ReceiverBatch(n_ch, max_len=max(RAGGED))
    b.set_option("pll_variant", variant)
    assert b.info("frame_times") == 0
    b.frame_times(True)
    assert b.info("frame_times") == 1
    ref = ftr.FrameTimeRef(n_ch)
    cuts = np.cumsum([0] + RAGGED)
    n_frames = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e])
        ref.run(x[a:e])
        assert b.info("rows") == e
        n_frames += len(check_drain(b, ref)[0])
    assert n_frames > 20 * n_ch
    b.reset()
    ref.reset()
    assert b.info("rows") == 0 and b.info("frame_times") == 1
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e], sync=False)
        ref.run(x[a:e])
    fr, t = check_drain(b, ref)
    assert len(fr) == n_frames and t.min() >= 0 and t.max() < total


def test_times_192k_table():
    from gnuais_amd import ReceiverBatch
    n_ch, calls = 5, [1, 777, 2047, 2048, 2049, 30000, 12000]
    total = sum(calls)
    x = tiled(n_ch, total, sps=20, n_base=5)
    b = ReceiverBatch(n_ch, taps=params.taps_192k(), pllinc=params.PLLINC_192K, max_len=max(calls))
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch, params.taps_192k(), params.PLLINC_192K)
    cuts = np.cumsum([0] + calls)
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(dev(x[a:e]), sync=False)
        ref.run(x[a:e])
    fr, _ = check_drain(b, ref)
    assert len(fr) >= 10
    assert b.time_map("audio") == ftr.time_map("audio", n_taps=144)


@pytest.mark.parametrize("variant", [7, 8])
def test_times_at_sixteen_samples_per_bit(variant):
    """pllinc 4096: the phase is a multiple of the nudge at every sample and meets the loop's equalities (pll == 0x8000 at
    a transition, == 0x10000 at a slice; tests/test_pll_cpu.py counts them), the segments hold 128 bits instead of 410.
    The stream of tests/test_pll_gpu.py's message test, ragged calls, both PLL forms: frames and times == restatement."""
    from gnuais_amd import ReceiverBatch
    n_ch, sps = 6, 16
    total = 30 * 256 * sps
    x = np.stack([synth.make_stream(total, seed=31, channel=c, sps=sps, sigma=1000)[0] for c in range(n_ch)], axis=1)
    calls = [1, 777, 2047, 2048, 2049, 48000]
    calls.append(total - sum(calls))
    b = ReceiverBatch(n_ch, pllinc=0x10000 // sps, max_len=max(calls))
    b.set_option("pll_variant", variant)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch, None, 0x10000 // sps)
    cuts = np.cumsum([0] + calls)
    n_frames = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(dev(x[a:e]))
        ref.run(x[a:e])
        assert b.info("pll_form") == (variant if e - a >= 256 else 8)
        fr, t = check_drain(b, ref)
        n_frames += len(fr)
        assert len(t) == 0 or (t.min() >= 0 and t.max() < e)
    assert n_frames >= 85


@pytest.mark.parametrize("W", [0, 1024])
def test_times_run_iq(W):
    from gnuais_amd import ReceiverBatch
    n_ch, total = 29, 16 * 1280
    x = np.stack([synth.make_iq_stream(total, seed=3, channel=c, sigma=800.0, occupancy=0.8, gated=True,
                                       offset_hz=3000.0 if W else 0.0)[0] for c in range(n_ch)], axis=1)
    calls = [1020, 1, 4096, 333, 7000]
    calls.append(total - sum(calls))
    b = ReceiverBatch(n_ch, max_len=max(calls))
    if W:
        b.afc(W)
    b.frame_times(True)
    ref, afc, carry = ftr.FrameTimeRef(n_ch), (afc_ref.Afc(n_ch, W) if W else None), None
    pos = 0
    for i, n in enumerate(calls):
        seg = x[pos:pos + n]
        pos += n
        b.run_iq(dev(seg), sync=False)
        if afc:
            audio = afc.apply(seg)
        else:
            audio, carry = iq_ref.discriminate(seg, carry)
        ref.run(audio)
        if i == 2:
            check_drain(b, ref)
    fr, _ = check_drain(b, ref)
    assert len(fr) > 100
    assert b.time_map("iq") == ftr.time_map("iq", afc_window=W)


@pytest.mark.parametrize("fmt,W", [("cs16", 0), ("cu8", 0), ("cs16", 1024)])
def test_times_run_wideband(fmt, W):
    from gnuais_amd import ReceiverBatch
    M, D, offs = 5, 6, (-25000, 25000)
    N, n = M * len(offs), 12 * 1280 * D
    x16 = np.stack([synth.make_wideband_stream(n, D, 48000 * D, offs, seed=3, stream=s, amplitude=1500.0, sigma=225.0,
                                               occupancy=0.8, gated=True, offset_hz=2500.0 if W else 0.0)[0]
                    for s in range(M)], axis=1)
    x = quantise(x16, fmt) if fmt != "cs16" else x16
    v = convert(x, fmt) if fmt != "cs16" else x16
    calls = [D * 1020, D, D * 4096, D * 333]
    calls.append(n - sum(calls))
    b = ReceiverBatch(N, max_len=max(calls) // D)
    b.channeliser(D, 48000 * D, offs)
    if W:
        b.afc(W)
    b.frame_times(True)
    ch, afc, carry = chan_ref.Channeliser(M, D, 48000 * D, offs), (afc_ref.Afc(N, W) if W else None), None
    ref = ftr.FrameTimeRef(N)
    pos = 0
    for c in calls:
        b.run_wideband(dev(x[pos:pos + c]), sync=False, fmt=None if fmt == "cs16" else fmt)
        iq = ch.run(v[pos:pos + c])
        if afc:
            audio = afc.apply(iq)
        else:
            audio, carry = iq_ref.discriminate(iq, carry)
        ref.run(audio)
        pos += c
    fr, _ = check_drain(b, ref)
    assert len(fr) > 60
    assert b.time_map("wideband") == ftr.time_map("wideband", afc_window=W, decim=D, chan_taps=16 * D + 1)


def test_times_with_a_stream_change_between_calls():
    """every call on another stream and nothing synchronised by the caller"""
    import torch
    from gnuais_amd import ReceiverBatch
    n_ch, rows, n_calls = 64, 3000, 7
    x = tiled(n_ch, rows * n_calls)
    xd = dev(x)
    b = ReceiverBatch(n_ch, max_len=rows)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch)
    streams = [torch.cuda.Stream() for _ in range(3)]
    for i in range(n_calls):
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            b.run(xd[i * rows:(i + 1) * rows], sync=False)
        ref.run(x[i * rows:(i + 1) * rows])
    fr, _ = check_drain(b, ref)
    torch.cuda.synchronize()
    assert len(fr) > 64 * 10


def test_times_across_reset_and_protodec_reset_in_mid_frame():
    from gnuais_amd import ReceiverBatch
    n_ch = 9
    x = tiled(n_ch, 8 * 1280, n_base=9)
    b = ReceiverBatch(n_ch, max_len=6000)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch)
    b.run(dev(x[:700]))                                        # 700 rows: first bursts (1190 rows long) are under way
    ref.run(x[:700])
    assert np.isin(b.fsm_state()["state"], (4, 5)).any()        # ST_DATA / ST_STOPSIGN: a frame is under way
    b.protodec_reset()
    ref.protodec_reset()
    assert b.info("rows") == 700                               # rows and the bit count stay
    for lo, hi in ((700, 4700), (4700, 8 * 1280)):
        b.run(dev(x[lo:hi]), sync=False)
        ref.run(x[lo:hi])
    fr, t = check_drain(b, ref)
    assert len(fr) > 20
    b.reset()
    ref.reset()
    b.run(dev(x[:4000]))
    ref.run(x[:4000])
    fr, t = check_drain(b, ref)
    assert len(fr) > 10 and t.max() < 4000


def test_decode_bits_gives_minus_one_between_timed_calls():
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    n_ch = 6
    x = tiled(n_ch, 6 * 1280, n_base=6)
    bits = Oracle(n_ch).run(x, want_bits=True)["bits"]
    b = ReceiverBatch(n_ch, max_len=4000)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch)
    b.run(dev(x[:4000]))
    ref.run(x[:4000])
    b.decode_bits(bits)
    ref.decode_bits(bits)
    b.run(dev(x[4000:]))
    ref.run(x[4000:])
    assert b.info("rows") == 6 * 1280                          # bits without samples are not rows
    fr, t = check_drain(b, ref)
    assert (t == -1).sum() >= 2 * n_ch and (t >= 0).sum() >= 2 * n_ch


def test_feature_switched_on_after_calls_have_run():
    """frames appended while it was off (still queued) have -1; rows were counted all along"""
    from gnuais_amd import ReceiverBatch
    n_ch = 11
    x = tiled(n_ch, 10 * 1280, n_base=11)
    b = ReceiverBatch(n_ch, max_len=6000)                      # the last call is 5800 rows
    ref = ftr.FrameTimeRef(n_ch)
    b.run(dev(x[:5000]), sync=False)
    b.run(dev(x[5000:7000]), sync=False)
    ref.run(x[:5000])
    ref.run(x[5000:7000])
    f0, t0 = ref.drain()
    b.frame_times(True)
    assert b.info("rows") == 7000
    b.run(dev(x[7000:]), sync=False)
    ref.run(x[7000:])
    f1, t1 = ref.drain()
    want_f = np.concatenate([f0, f1])
    want_t = np.concatenate([np.full(len(t0), -1, dtype=np.int64), t1])
    order = np.lexsort((ftr.stamp(want_f), want_f["channel"]))
    fr, t = b.drain_frames_timed()
    assert fr.tobytes() == want_f[order].tobytes() and np.array_equal(t, want_t[order])
    assert len(f0) > 20 and len(f1) > 10 and t1.min() >= 7000


def test_node_of_four_shards():
    from gnuais_amd import ReceiverBatch, ReceiverNode
    n_ch, rows = 101, 5000
    x = tiled(n_ch, 3 * rows)
    nd = ReceiverNode(n_ch, devices=[0, 0, 0, 0], max_len=rows)
    b = ReceiverBatch(n_ch, max_len=rows)
    nd.frame_times(True)
    ref = ftr.FrameTimeRef(n_ch)
    for lo in range(0, 3 * rows, rows):
        nd.run_host(x[lo:lo + rows])
        b.run(x[lo:lo + rows])
        ref.run(x[lo:lo + rows])
    nd.sync()
    fr, t = nd.drain_frames_timed()
    wf, wt = ref.drain()
    assert fr.tobytes() == wf.tobytes() == b.drain_frames().tobytes() and np.array_equal(t, wt) and len(fr) > 101 * 5
    assert nd.time_map("audio") == (1, -18)
    nd.close()


def test_one_c3_size_call():
    """16384 channels x 48000 rows in one call, tiled from 256 base streams as bench.py tiles them.  The frames of ALL
    channels equal the plain drain of a second batch; the times of 1024 channels (every 16th: what the single-threaded
    oracle does in a few seconds) equal the restatement, and every time lies inside the call."""
    import torch
    from gnuais_amd import ReceiverBatch, tile_channels
    n_ch, rows, step = 16384, 48000, 16
    base, _ = synth.make_base_streams(256, rows, seed=11, occupancy=0.8)
    xd = tile_channels(dev(base), n_ch)
    a = ReceiverBatch(n_ch, max_len=rows)
    a.frame_times(True)
    a.run(xd)
    fr, t = a.drain_frames_timed()
    del a
    p = ReceiverBatch(n_ch, max_len=rows)
    p.run(xd)
    assert fr.tobytes() == p.drain_frames().tobytes() and len(fr) > 20 * n_ch          # 37.5 slots at 0.8 occupancy: about 29 a channel
    del p
    assert t.min() >= 0 and t.max() < rows
    sel = np.arange(0, n_ch, step)
    ref = ftr.FrameTimeRef(len(sel))
    ref.run(xd[:, ::step].cpu().numpy())
    wf, wt = ref.drain()
    pick = fr["channel"] % step == 0
    got_f = fr[pick].copy()
    got_f["channel"] //= step
    assert got_f.tobytes() == wf.tobytes() and np.array_equal(t[pick], wt) and len(wf) > 20 * len(sel)


def test_feature_off_is_a_batch_that_never_enabled_it_and_the_state_errors():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import GnuaisError, E_STATE
    n_ch = 40
    x = tiled(n_ch, 3 * 4000)
    xd = dev(x)
    never, was = ReceiverBatch(n_ch, max_len=4000), ReceiverBatch(n_ch, max_len=4000)
    with pytest.raises(GnuaisError) as e:
        was.drain_frames_timed()
    assert e.value.code == E_STATE
    was.frame_times(True)
    was.run(xd[:4000])
    # the plain drains keep working while it is on
    seq = np.zeros(n_ch, dtype=np.uint8)
    assert was.pending_frames() > 0
    text, n_sent, n_fr = was.drain_nmea(seq)
    assert n_fr > 20 and text.count(b"!AIVDM") == n_sent
    # while it is on the batch does not start streaming
    for call in (was.stream_nmea, lambda: was.set_option("streaming", 1)):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    was.frame_times(False)
    was.reset()
    for lo in range(0, 3 * 4000, 4000):
        never.run(xd[lo:lo + 4000], sync=False)
        was.run(xd[lo:lo + 4000], sync=False)
    never.sync()
    was.sync()
    got = frames_state(was)
    assert got == frames_state(never) and len(got[0]) > 64 * 100
    with pytest.raises(GnuaisError) as e:
        was.drain_frames_timed()
    assert e.value.code == E_STATE
    # a streaming batch refuses the feature
    never.stream_nmea()
    with pytest.raises(GnuaisError) as e:
        never.frame_times(True)
    assert e.value.code == E_STATE
    never.set_option("streaming", 0)
    never.frame_times(True)
    assert never.info("frame_times") == 1


def test_decode_file_times_prints_the_tags_of_the_cpu_formatter(tmp_path):
    """decode_file.py --wideband 6 --times --start S on a generated .cu8 capture: the sentences of the run without
    --times, each behind the tag the CPU restatement and the CPU formatter give for it"""
    from gnuais_amd import nmea_tagged_from_frames
    D, R, offs, M, start, call = 6, 288000, (-25000, 25000), 2, 1_700_000_000, 5000
    n = 10 * 1280 * D
    x16 = np.stack([synth.make_wideband_stream(n, D, R, offs, seed=9, stream=s, amplitude=1500.0, sigma=225.0,
                                               occupancy=0.8)[0] for s in range(M)], axis=1)
    x = quantise(x16, "cu8")
    path = str(tmp_path / "capture.cu8")
    x.tofile(path)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), path, "--wideband", str(D),
                                     "--rate", str(R), "--streams", str(M), "--call", str(call), *a],
                                    check=True, capture_output=True, timeout=300)        # bytes: "\r\n" stays
    plain, got = run(), run("--times", "--start", str(start))
    N = M * len(offs)
    ref, ch, carry = ftr.FrameTimeRef(N), chan_ref.Channeliser(M, D, R, offs), None
    seq = np.zeros(N, dtype=np.uint8)
    mul, off = ftr.time_map("wideband", decim=D, chan_taps=16 * D + 1)
    want = b""
    v = convert(x, "cu8")
    for lo in range(0, n, call * D):
        audio, carry = iq_ref.discriminate(ch.run(v[lo:lo + call * D]), carry)
        ref.run(audio)
        fr, t = ref.drain()
        want += nmea_tagged_from_frames(fr, t, seq, mul, off, R, start)
    assert got.stdout == want and got.stdout.count(b"\\c:17000000") > 30
    import re
    assert re.sub(rb"\\c:\d+\*[0-9A-F]{2}\\", b"", got.stdout) == plain.stdout and plain.stdout.count(b"!AIVDM") > 30
