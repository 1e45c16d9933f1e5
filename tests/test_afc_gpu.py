"""The carrier-error stage (AFC) on the device: gnuais_batch_afc_apply and _afc_estimate bit for bit against the NumPy
restatement of the definition (tests/afc_ref.py), and run_iq / run_wideband with the AFC on = run on the restated
audio = the CPU oracle, on bursts whose carrier is kHz off."""
import os
import subprocess
import sys

import numpy as np
import pytest

import afc_ref
import chan_ref
import iq_ref
from gnuais_amd import synth
from test_iq_gpu import dev, frames_state, hard_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def hard_stream(rng, n_rows, n_ch):
    """hard_pairs with stretches that make the window sums large and of either sign: full-scale tones of a few
    frequencies per channel (sums near 2^45: the fp32 conversion rounds), the all -32768 pair (r = 2^31), silence"""
    x = hard_pairs(rng, n_rows, n_ch)
    t = np.arange(n_rows)[:, None]
    w = rng.uniform(-np.pi, np.pi, n_ch)[None, :]
    tone = np.stack([np.rint(32767 * np.cos(w * t)), np.rint(32767 * np.sin(w * t))], axis=-1).astype(np.int16)
    kind = rng.integers(0, 5, (max(n_rows // 97, 1) + 1, n_ch))      # per stretch of 97 rows and channel
    kind = np.repeat(kind, 97, axis=0)[:n_rows]
    x[kind == 1] = tone[kind == 1]
    x[kind == 2] = -32768
    x[kind == 3] = 0
    return x


CASES = [(n, W) for n in (1, 3, 65, 1000, 4096) for W in (128, 1024)] + [(3, 16384), (65, 16384), (1000, 16384)]


@pytest.mark.parametrize("n_ch,W", CASES)
def test_afc_apply_and_estimate_bit_exact_ragged_and_reset(n_ch, W):
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(1000 * n_ch + W)
    chunks = [1, 63, 64, 65, 200, 1, 129, 700] if n_ch <= 1000 else [1, 130, 64, 257, 600]
    if W == 16384:
        chunks += [9000, 3000, 4097, 5000]
    x = hard_stream(rng, sum(chunks) * 2, n_ch)
    b = ReceiverBatch(n_ch, max_len=max(chunks))
    assert b.info("afc_window") == 0
    b.afc(W)
    assert b.info("afc_window") == W
    ref = afc_ref.Afc(n_ch, W)
    assert np.array_equal(b.afc_estimate(), ref.estimate())
    pos = 0
    for rep in range(2):
        for n in chunks if rep == 0 else chunks[::-1]:
            seg = x[pos:pos + n]
            pos += n
            got = b.afc_apply(dev(seg)).cpu().numpy()
            want = ref.apply(seg)
            assert got.dtype == np.int16 and got.shape == (n, n_ch)
            assert np.array_equal(got, want), (n_ch, W, rep, n, np.argwhere(got != want)[:5])
            assert np.array_equal(b.afc_estimate(), ref.estimate()), (rep, n)
        assert np.any(want != 0)
        b.reset()                                        # in the middle of the stream: the state is zero, the window kept
        ref.reset()
        assert b.info("afc_window") == W and not b.afc_estimate().any()
    assert pos == x.shape[0]


def test_afc_arguments_and_off_state():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import GnuaisError, E_ARG, E_STATE
    b = ReceiverBatch(4, max_len=256)
    for bad in (-128, 64, 127, 192, 1000, 16384 + 128, 32768):
        with pytest.raises(GnuaisError) as e:
            b.afc(bad)
        assert e.value.code == E_ARG, bad
    x = dev(np.zeros((10, 4, 2), dtype=np.int16))
    for call in (lambda: b.afc_apply(x), b.afc_estimate):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == E_STATE
    b.afc(128)
    b.afc(0)
    with pytest.raises(GnuaisError):
        b.afc_estimate()


def test_afc_apply_unaligned_views():
    """input and output views that start one channel in: the narrow lane forms; the same numbers"""
    from gnuais_amd import ReceiverBatch
    import torch
    rng = np.random.default_rng(9)
    n_ch, rows, W = 64, 700, 256
    x = hard_stream(rng, rows, n_ch + 1)
    whole = dev(x.reshape(-1)).view(torch.int16)
    part = whole[2:2 + rows * n_ch * 2].view(rows, n_ch, 2)              # not 16-byte aligned
    want = afc_ref.apply_stream(part.cpu().numpy(), W, [300, 400])
    b = ReceiverBatch(n_ch, max_len=rows)
    b.afc(W)
    got = torch.cat([b.afc_apply(part[:300]), b.afc_apply(part[300:])]).cpu().numpy()
    assert np.array_equal(got, want)
    # the output at an odd int16 offset, through the C entry
    b.reset()
    out = torch.zeros(rows * n_ch + 1, dtype=torch.int16, device=part.device)
    from gnuais_amd.lib import check
    import ctypes as C
    for lo, hi in ((0, 300), (300, rows)):
        seg = part[lo:hi].contiguous()
        check(b._lib.gnuais_batch_afc_apply(b._h, seg.data_ptr(), hi - lo, out.data_ptr() + 2 * (1 + lo * n_ch),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(out[1:].view(rows, n_ch).cpu().numpy(), want) and int(out[0]) == 0


def offset_streams(n_ch, total, offset_hz, seed=3, sigmas=(300.0, 800.0, 1500.0)):
    """gated bursts; channel c is offset_hz + 100 c Hz off.  Every channel holds noise between the bursts, as a real one
    does (exact silence there is another matter: DESIGN.md 4.10)"""
    made = [synth.make_iq_stream(total, seed=seed, channel=c, sigma=sigmas[c % len(sigmas)], occupancy=0.8, gated=True,
                                 offset_hz=offset_hz + 100.0 * c) for c in range(n_ch)]
    return np.stack([m[0] for m in made], axis=1), [m[1] for m in made]


def complete(placed, total, W):
    """the placed bursts that the chain has seen whole: the AFC holds back the stream's last W/2 samples"""
    return sum(1 for p in placed for slot, _ in p if (slot + 1) * 1280 + W // 2 <= total)


def counters3(b):
    cnt = b.counters()
    return np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1)


def test_run_iq_with_afc_equals_run_on_restated_audio_and_the_oracle():
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    n_ch, W = 29, 1024
    total = 24 * synth.SLOT_BITS * 5
    x, placed = offset_streams(n_ch, total, 4000.0)
    chunks = [1020, 1, 4096, 333, 7000]
    chunks.append(total - sum(chunks))
    a = ReceiverBatch(n_ch, max_len=max(chunks))
    r = ReceiverBatch(n_ch, max_len=max(chunks))
    a.afc(W)
    ref = afc_ref.Afc(n_ch, W)
    o = Oracle(n_ch)
    pos = 0
    for n in chunks:                                     # pipelined: no sync between the calls
        seg = x[pos:pos + n]
        pos += n
        audio = ref.apply(seg)
        a.run_iq(dev(seg), sync=False)
        r.run(dev(audio), sync=False)
        o.run(audio)
    a.sync()
    r.sync()
    # the estimates at the end: each channel's own error, in Hz within the estimator's noise
    est = a.afc_estimate()
    assert np.array_equal(est, ref.estimate())
    got, want = frames_state(a), frames_state(r)
    assert got == want
    assert got[0] == o.frames().tobytes()
    assert np.array_equal(counters3(a), o.counters())
    n_placed = complete(placed, total, W)
    assert counters3(a)[:, 0].sum() >= 0.9 * n_placed and n_placed > 400
    # the same batch with the AFC off decodes none of them; the host form
    a.afc(0)
    a.reset()
    a.run_iq(x[:max(chunks)])
    a.run_iq(x[max(chunks):2 * max(chunks)])
    assert counters3(a)[:, 0].sum() == 0 and len(a.drain_frames()) == 0
    # AFC off after it was on: the bits of a batch that never had it (on input it can decode)
    never = ReceiverBatch(n_ch, max_len=max(chunks))
    y = np.stack([synth.make_iq_stream(total, seed=5, channel=c, sigma=800.0, occupancy=0.8, gated=True)[0]
                  for c in range(n_ch)], axis=1)
    a.reset()
    pos = 0
    for n in chunks:
        a.run_iq(dev(y[pos:pos + n]), sync=False)
        never.run_iq(dev(y[pos:pos + n]), sync=False)
        pos += n
    a.sync()
    never.sync()
    got = frames_state(a)
    assert got == frames_state(never) and len(got[0]) > 64 * 200


def test_run_wideband_mistuned_with_afc_equals_the_oracle():
    """the offsets the channeliser is given are 3 kHz off the channels' true places"""
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    M, K, D, W = 9, 2, 6, 1024
    N = M * K
    n = 16 * synth.SLOT_BITS * 5 * D
    true = (-25000, 25000)
    tuned = [f - 3000 for f in true]                     # the receiver believes the channels 3 kHz lower: error +3 kHz
    made = [synth.make_wideband_stream(n, D, 48000 * D, true, seed=3, stream=s, sigma=500.0, occupancy=0.8, gated=True)
            for s in range(M)]
    x = np.stack([m[0] for m in made], axis=1)
    n_placed = complete([p for m in made for p in m[1]], n // D, W)
    chunks = [D * 1020, D, D * 4096, D * 333]
    chunks.append(n - sum(chunks))
    a = ReceiverBatch(N, max_len=max(chunks) // D)
    a.channeliser(D, 48000 * D, tuned)
    a.afc(W)
    cref = chan_ref.Channeliser(M, D, 48000 * D, tuned)
    ref = afc_ref.Afc(N, W)
    o = Oracle(N)
    pos = 0
    for c in chunks:
        a.run_wideband(dev(x[pos:pos + c]), sync=False)
        o.run(ref.apply(cref.run(x[pos:pos + c])))
        pos += c
    a.sync()
    est = a.afc_estimate()
    assert np.array_equal(est, ref.estimate())
    got = frames_state(a)
    assert got[0] == o.frames().tobytes()
    assert np.array_equal(counters3(a), o.counters())
    assert counters3(a)[:, 0].sum() >= 0.9 * n_placed and n_placed > 150
    # without the AFC the mistuned batch decodes nothing
    a.afc(0)
    a.reset()
    a.run_wideband(x[:chunks[2]])
    assert counters3(a)[:, 0].sum() == 0


def test_mixed_calls_and_stream_changes_with_afc():
    """audio, I/Q and wideband calls in turn on one batch with the AFC on, every call on another stream and nothing
    synchronised by the caller (the drain rule), against the same calls on one stream; the audio calls leave the AFC
    state alone, and the I/Q-type calls share it"""
    import torch
    from gnuais_amd import ReceiverBatch
    M, K, D, W = 64, 2, 6, 256
    N = M * K
    rows = 3000
    n_calls = 9
    iq, _ = offset_streams(N, rows * n_calls, 2500.0, sigmas=(500.0,))
    made = [synth.make_wideband_stream(rows * D * n_calls, D, 48000 * D, (-25000, 25000), seed=8, stream=s, sigma=500.0,
                                       occupancy=0.8, gated=True, offset_hz=-2000.0) for s in range(M)]
    wide = np.stack([m[0] for m in made], axis=1)
    audio = np.stack([synth.make_stream(rows * n_calls, seed=2, channel=c, occupancy=0.8)[0] for c in range(N)], axis=1)
    iqd, wided, audiod = dev(iq), dev(wide), dev(audio)
    one = ReceiverBatch(N, max_len=rows)
    many = ReceiverBatch(N, max_len=rows)
    for b in (one, many):
        b.channeliser(D, 48000 * D, [-25000, 25000])
        b.afc(W)
    cref = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000])
    ref = afc_ref.Afc(N, W)
    streams = [torch.cuda.Stream() for _ in range(3)]

    def call(b, i):
        lo = i * rows
        if i % 3 == 0:
            b.run(audiod[lo:lo + rows], sync=False)
        elif i % 3 == 1:
            b.run_iq(iqd[lo:lo + rows], sync=False)
        else:
            b.run_wideband(wided[lo * D:(lo + rows) * D], sync=False)

    for i in range(n_calls):
        call(one, i)
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            call(many, i)
        lo = i * rows
        if i % 3 == 1:
            ref.apply(iq[lo:lo + rows])
        elif i % 3 == 2:
            ref.apply(cref.run(wide[lo * D:(lo + rows) * D]))
    one.sync()
    many.sync()
    torch.cuda.synchronize()
    assert np.array_equal(one.afc_estimate(), ref.estimate())
    assert np.array_equal(many.afc_estimate(), ref.estimate())
    assert frames_state(one) == frames_state(many)
    assert one.counters()["receivedframes"].sum() > 200


def test_node_two_shards_with_afc_equal_one_batch():
    from gnuais_amd import ReceiverBatch, ReceiverNode
    n_ch, total, W = 101, 10 * 1280, 1024
    x, _ = offset_streams(n_ch, total, -12500.0)             # -12.5 .. -2.5 kHz: none decodes uncorrected
    nd = ReceiverNode(n_ch, devices=[0, 0], max_len=5000)
    b = ReceiverBatch(n_ch, max_len=5000)
    nd.afc(W)
    b.afc(W)
    for mode in ("host", "device"):
        for lo in range(0, total, 5000):
            if mode == "host":
                nd.run_iq_host(x[lo:lo + 5000])
            else:
                nd.run_iq([dev(x[lo:lo + 5000, f:f + n], d) for d, f, n in nd.shards])
            b.run_iq(x[lo:lo + 5000])
        nd.sync()
        assert nd.drain_frames().tobytes() == b.drain_frames().tobytes()
        assert nd.counters().tobytes() == b.counters().tobytes()
        assert nd.pll_state().tobytes() == b.pll_state().tobytes()
        assert b.counters()["receivedframes"].sum() > 150
        nd.reset()
        b.reset()
    nd.afc(0)
    nd.run_iq_host(x[:5000])
    nd.sync()
    assert nd.counters()["receivedframes"].sum() == 0
    nd.close()


def test_decode_file_iq_afc_equals_the_audio_path(tmp_path):
    from gnuais_amd import io
    W = 1024
    x, _ = offset_streams(2, 20 * 1280, 4000.0, sigmas=(1000.0,))
    iq_path, au_path = str(tmp_path / "iq.wav"), str(tmp_path / "audio.wav")
    io.write_wav(iq_path, 48000, x.reshape(x.shape[0], 4))                  # 2 receivers = 4 channels: I0 Q0 I1 Q1
    flushed = np.concatenate([x, np.zeros((W // 2, 2, 2), dtype=np.int16)])  # decode_file pushes the delay through
    io.write_wav(au_path, 48000, afc_ref.apply_stream(flushed, W))
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), *a, "--call", "5000"],
                                    check=True, capture_output=True, text=True, timeout=300)
    got, want, off = run(iq_path, "--iq", "--afc", str(W)), run(au_path), run(iq_path, "--iq")
    assert got.stdout == want.stdout and got.stdout.count("!AIVDM") > 20
    assert off.stdout.count("!AIVDM") == 0
    hz = [float(v) for v in got.stderr.strip().splitlines()[-1].split(":")[1].split()]
    assert len(hz) == 2


def test_decode_file_wideband_afc_equals_the_audio_path(tmp_path):
    from gnuais_amd import io
    D, M, W = 6, 2, 1024
    true = (-25000, 25000)
    n = 10 * 1280 * D
    x = np.stack([synth.make_wideband_stream(n, D, 48000 * D, true, seed=3, stream=s, sigma=500.0, occupancy=0.8,
                                             gated=True, offset_hz=2500.0)[0] for s in range(M)], axis=1)
    flushed = np.concatenate([x, np.zeros((W // 2 * D, M, 2), dtype=np.int16)])   # decode_file pushes the delay through
    audio = afc_ref.apply_stream(chan_ref.Channeliser(M, D, 48000 * D, true).run(flushed), W)
    wide_path, au_path = str(tmp_path / "wide.wav"), str(tmp_path / "audio.wav")
    io.write_wav(wide_path, 48000 * D, x.reshape(x.shape[0], 2 * M))
    io.write_wav(au_path, 48000, audio)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), *a, "--call", "5000"],
                                    check=True, capture_output=True, text=True, timeout=300)
    got, want = run(wide_path, "--wideband", str(D), "--afc", str(W)), run(au_path)
    assert got.stdout == want.stdout and got.stdout.count("!AIVDM") > 20
    assert run(wide_path, "--wideband", str(D)).stdout.count("!AIVDM") == 0
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), au_path, "--afc", str(W)],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--afc needs --iq or --wideband" in bad.stderr


def test_c3_shape_afc_apply_every_channel():
    """16384 channels x 48000 rows of full-range random pairs in one call, W = 1024: bands of rows at the start, in the
    middle and at the end compared on every channel (a fresh restatement started on a block of n at least W rows
    before a band gives the band's bits: nothing older enters its windows)."""
    import torch
    from gnuais_amd import ReceiverBatch
    n_ch, total, W = 16384, 48000, 1024
    g = torch.Generator(device="cuda:0").manual_seed(11)
    xd = torch.randint(-32768, 32767, (total, n_ch, 2), dtype=torch.int16, device="cuda:0", generator=g)
    xd[20000:23000, ::3] = -32768                       # r = 2^31 over whole windows on every third channel
    b = ReceiverBatch(n_ch, max_len=total)
    b.afc(W)
    out = b.afc_apply(xd)
    est = b.afc_estimate()
    for lo, hi in ((0, 700), (21_000, 21_300), (total - 200, total)):
        s0 = max((lo - W) // 64 * 64, 0)
        ref = afc_ref.Afc(n_ch, W)
        if s0:
            ref.carry = xd[s0 - 1].cpu().numpy()
        want = ref.apply(xd[s0:hi].cpu().numpy())[lo - s0:]
        assert np.array_equal(out[lo:hi].cpu().numpy(), want), lo
    assert np.array_equal(est, ref.estimate())
