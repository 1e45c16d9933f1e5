"""Wideband in, on the device: gnuais_batch_channelise bit for bit against the NumPy restatement of its definition
(tests/chan_ref.py), and gnuais_batch_run_wideband = gnuais_batch_run_iq on the restated I/Q = the CPU oracle."""
import numpy as np
import pytest

import chan_ref
import iq_ref
from gnuais_amd import synth

pytestmark = pytest.mark.gpu
R6 = 288000
OFFS = {1: [25000], 2: [-25000, 25000], 3: [-25000, 0, 25000]}


def dev(x, device=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")


def hard_wide(rng, n_rows, M):
    x = rng.integers(-32768, 32768, (n_rows, M, 2)).astype(np.int16)
    special = np.array([32767, -32768, -32767, 0], dtype=np.int16)
    m = rng.random((n_rows, M)) < 0.25
    x[m] = rng.choice(special, (int(m.sum()), 2))
    return x


@pytest.mark.parametrize("M,K,D", [(1, 1, 1), (3, 2, 2), (65, 3, 6), (65, 2, 8), (3, 3, 8), (4096, 2, 6), (1, 2, 6)])
def test_channelise_bit_exact_ragged_and_reset(M, K, D):
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(M * 100 + K * 10 + D)
    chunks = [1, 37, 300, 2, 129] if M < 4096 else [5, 400]
    chunks = [c * D for c in chunks]
    x = hard_wide(rng, sum(chunks), M)
    b = ReceiverBatch(M * K, max_len=max(chunks) // D)
    b.channeliser(D, 48000 * D, OFFS[K])
    ref = chan_ref.Channeliser(M, D, 48000 * D, OFFS[K])
    for rep in range(2):
        pos = 0
        for n in chunks:
            got = b.channelise(dev(x[pos:pos + n])).cpu().numpy()
            want = ref.run(x[pos:pos + n])
            pos += n
            assert got.shape == (n // D, M * K, 2)
            assert np.array_equal(got, want), (M, K, D, rep, n, np.argwhere(got != want)[:5])
        b.reset()                                       # carry and n are zero again, the configuration stays
        ref.reset()


@pytest.mark.parametrize("taps_kind", ["bound", "long", "odd"])
def test_custom_taps_at_the_sum_bound(taps_kind):
    """sum |h| = 65535 with full-scale input: the fast form (short filters) and the direct form (long ones)"""
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(3)
    if taps_kind == "bound":
        D, h = 2, np.array([32767, -32767, 1], dtype=np.int16)
    elif taps_kind == "long":
        D, h = 1, np.zeros(300, dtype=np.int16)  # ceil(T / D) = 300 accumulators: the direct form
        h[::3] = 327
        h[3::6] = -327
        h[1], h[2] = 32767, 68                   # sum |h| = 100 * 327 + 32767 + 68 = 65535
    else:
        D, h = 3, rng.integers(-600, 600, 61).astype(np.int16)
    assert np.abs(h.astype(np.int64)).sum() <= 65535
    M, K = 65, 2
    x = hard_wide(rng, D * 700, M)
    x[: D * 50] = -32768
    b = ReceiverBatch(M * K, max_len=700)
    b.channeliser(D, 48000 * D, [-25000, 25000], taps=h)
    ref = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000], taps=h)
    for lo, hi in ((0, D * 3), (D * 3, D * 400), (D * 400, D * 700)):
        assert np.array_equal(b.channelise(dev(x[lo:hi])).cpu().numpy(), ref.run(x[lo:hi])), (taps_kind, lo)


def test_bad_configurations_and_calls_are_refused():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import GnuaisError
    b = ReceiverBatch(6, max_len=100)
    x = dev(np.zeros((12, 3, 2), dtype=np.int16))
    with pytest.raises(GnuaisError, match="no channeliser configured"):
        b.run_wideband(x)
    bad = [dict(decim=0), dict(decim=65), dict(offsets_hz=[1, 2, 3, 4]), dict(offsets_hz=[1]),
           dict(in_rate_hz=(1 << 20) + 1, offsets_hz=[1, 1]), dict(taps=np.zeros(1026, dtype=np.int16)),
           dict(taps=np.array([-32768], dtype=np.int16)), dict(taps=np.array([32767, 32767, 2], dtype=np.int16))]
    for kw in bad:
        args = dict(decim=2, in_rate_hz=96000, offsets_hz=[-25000, 25000])
        args.update(kw)
        if args["offsets_hz"] == [1]:
            b2 = ReceiverBatch(6, max_len=100)
            b2.channeliser(**args)                      # K = 1 with 6 streams: allowed
            continue
        with pytest.raises(GnuaisError):
            b.channeliser(**args)
    b.channeliser(4, 192000, [-25000, 25000])
    with pytest.raises(GnuaisError, match="multiple of the decimation"):
        b._wide_shape_ok = lambda *a: True
        b.run_wideband(dev(np.zeros((6, 3, 2), dtype=np.int16)))
    with pytest.raises(GnuaisError):
        b.run_wideband(dev(np.zeros((404, 3, 2), dtype=np.int16)))      # more than D * max_len


def frames_state(b):
    cnt = b.counters()
    return (b.drain_frames().tobytes(), cnt.tobytes(), b.pll_state().tobytes(), b.fsm_state().tobytes(),
            b.maxval().tobytes())


def wide_streams(M, n, D=6, offs=(-25000, 25000), seed=3, sigma=500.0):
    made = [synth.make_wideband_stream(n, D, 48000 * D, offs, seed=seed, stream=s, sigma=sigma, occupancy=0.8)
            for s in range(M)]
    return np.stack([m[0] for m in made], axis=1), [m[1] for m in made]


def test_run_wideband_equals_run_iq_and_the_oracle():
    """End to end at D = 6, K = 2, 64 streams: frames, counters and PLL state against run_iq on the restated I/Q, and
    the frames against the CPU oracle on the restated audio; calls mixed with run and run_iq on one batch."""
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    M, K, D = 64, 2, 6
    N = M * K
    n = 20 * synth.SLOT_BITS * 5 * D
    x, placed = wide_streams(M, n)
    chunks = [D * 1020, D, D * 4096, D * 333]
    chunks.append(n - sum(chunks))
    a = ReceiverBatch(N, max_len=max(chunks) // D)
    r = ReceiverBatch(N, max_len=max(chunks) // D)
    a.channeliser(D, 48000 * D, [-25000, 25000])
    ref = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000])
    o = Oracle(N)
    iq_all = []
    pos = 0
    for c in chunks:                                    # pipelined: no sync between the calls
        iq = ref.run(x[pos:pos + c])
        pos += c
        iq_all.append(iq)
        a.run_wideband(dev(x[pos - c:pos]), sync=False)
        r.run_iq(dev(iq), sync=False)
    a.sync()
    r.sync()
    got, want = frames_state(a), frames_state(r)
    assert got == want
    audio, _ = iq_ref.discriminate(np.concatenate(iq_all))
    o.run(audio)
    assert got[0] == o.frames().tobytes()
    cnt = a.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), o.counters())
    total = sum(len(p[k]) for p in placed for k in range(K))
    assert cnt["receivedframes"].sum() >= 0.95 * total and total > 1500
    # mixed with audio and run_iq calls on one batch: they leave the channeliser's state alone
    a.reset()
    r.reset()
    ref.reset()
    rng = np.random.default_rng(1)
    step = D * 4096
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        iq = ref.run(x[lo:hi])
        a.run_wideband(x[lo:hi])                        # the host form
        r.run_iq(iq)
        extra_iq = rng.integers(-3000, 3000, (500, N, 2)).astype(np.int16)
        extra_au = rng.integers(-3000, 3000, (700, N)).astype(np.int16)
        for bb in (a, r):
            bb.run_iq(extra_iq)
            bb.run(extra_au)
    assert frames_state(a)[:4] == frames_state(r)[:4]


def test_stream_change_between_run_wideband_calls():
    import torch
    from gnuais_amd import ReceiverBatch
    M, D = 128, 6
    n = 12 * 1280 * D
    x, _ = wide_streams(M, n, sigma=800.0)
    xd = dev(x)
    chunks = [D * 3000] * 5
    chunks.append(n - sum(chunks))
    one = ReceiverBatch(2 * M, max_len=3000)
    many = ReceiverBatch(2 * M, max_len=3000)
    for b in (one, many):
        b.channeliser(D, 48000 * D, [-25000, 25000])
    streams = [torch.cuda.Stream() for _ in range(3)]
    pos = 0
    for i, c in enumerate(chunks):
        one.run_wideband(xd[pos:pos + c], sync=False)
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            many.run_wideband(xd[pos:pos + c], sync=False)
        pos += c
    one.sync()
    many.sync()
    torch.cuda.synchronize()
    assert frames_state(one) == frames_state(many)
    assert one.counters()["receivedframes"].sum() > 1000


def test_node_two_shards_equal_one_batch_and_misaligned_shards_are_refused():
    from gnuais_amd import ReceiverBatch, ReceiverNode
    from gnuais_amd.lib import GnuaisError
    M, D = 50, 6
    n = 8 * 1280 * D
    x, _ = wide_streams(M, n)
    iq = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000]).run(x)
    audio = iq_ref.discriminate(iq)[0]
    nd = ReceiverNode(2 * M, devices=[0, 0], max_len=2000)
    b = ReceiverBatch(2 * M, max_len=2000)
    nd.channeliser(D, 48000 * D, [-25000, 25000])
    b.channeliser(D, 48000 * D, [-25000, 25000])
    # audio, I/Q and wideband calls in turn, narrowest first, so that the node's staging slab grows across the forms
    forms = ((nd.run_host, b.run, audio, 1), (nd.run_iq_host, b.run_iq, iq, 1),
             (nd.run_wideband_host, b.run_wideband, x, D))
    for i, lo in enumerate(range(0, n // D, 2000)):
        run_node, run_batch, src, rows = forms[i % 3]
        run_node(src[lo * rows:(lo + 2000) * rows])
        run_batch(src[lo * rows:(lo + 2000) * rows])
    nd.sync()
    assert nd.drain_frames().tobytes() == b.drain_frames().tobytes()
    assert nd.counters().tobytes() == b.counters().tobytes()
    assert nd.pll_state().tobytes() == b.pll_state().tobytes()
    assert b.counters()["receivedframes"].sum() > 200
    nd.close()
    odd = ReceiverNode(2 * 51, devices=[0, 0], max_len=100)          # shards of 51 channels: 51 % 2 != 0
    with pytest.raises(GnuaisError, match="shard 0"):
        odd.channeliser(D, 48000 * D, [-25000, 25000])
    odd.close()


def test_w3_shape_in_one_call():
    """8192 streams x K = 2 x D = 6, 288 000 wide samples in one call (C3's 16 384 x 48 000 out); 16 sampled streams
    bit for bit against the restatement, and all 8192 x 2 against chan_ref.torch_channelise, the same definition in
    torch's int64 operations on the device (pinned to the restatement by test_channeliser_cpu.py)."""
    import torch
    from gnuais_amd import ReceiverBatch
    M, K, D, n = 8192, 2, 6, 288000
    g = torch.Generator(device="cuda:0").manual_seed(7)
    xd = torch.randint(-32768, 32767, (n, M, 2), dtype=torch.int16, device="cuda:0", generator=g)
    b = ReceiverBatch(M * K, max_len=n // D)
    b.channeliser(D, 48000 * D, [-25000, 25000])
    out = b.channelise(xd)
    assert tuple(out.shape) == (n // D, M * K, 2)
    pick = np.random.default_rng(0).choice(M, 16, replace=False)
    pick.sort()
    sub = xd[:, torch.from_numpy(pick).to(xd.device)].cpu().numpy()
    want = chan_ref.Channeliser(16, D, 48000 * D, [-25000, 25000]).run(sub)
    cols = (pick[:, None] * K + np.arange(K)[None, :]).reshape(-1)
    got = out[:, torch.from_numpy(cols).to(out.device)].cpu().numpy()
    assert np.array_equal(got, want)
    del got, sub
    full = chan_ref.torch_channelise(xd, D, 48000 * D, [-25000, 25000], chan_ref.default_taps(D), chunk=512)
    assert full.shape == out.shape
    bad = int((full != out).sum())
    del full, out, xd
    torch.cuda.empty_cache()
    assert bad == 0, bad


def test_decode_file_wideband_equals_the_iq_path(tmp_path):
    import os
    import subprocess
    import sys
    from gnuais_amd import io
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    D, M = 6, 2
    x, _ = wide_streams(M, 10 * 1280 * D)
    iq = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000]).run(x)
    wide_path, iq_path = str(tmp_path / "wide.wav"), str(tmp_path / "iq.wav")
    io.write_wav(wide_path, 48000 * D, x.reshape(x.shape[0], 2 * M))
    io.write_wav(iq_path, 48000, iq.reshape(iq.shape[0], 4 * M))
    run = lambda *a: subprocess.run([sys.executable, os.path.join(root, "scripts", "decode_file.py"), *a, "--call", "5000"],
                                    check=True, capture_output=True, text=True, timeout=300)
    got, want = run(wide_path, "--wideband", str(D)), run(iq_path, "--iq")
    assert got.stdout == want.stdout and got.stdout.count("!AIVDM") > 10
