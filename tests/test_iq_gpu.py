"""Complex baseband in, on the device: gnuais_batch_discriminate bit for bit against the NumPy restatement of its
definition (tests/iq_ref.py), and gnuais_batch_run_iq = gnuais_batch_run on the restated audio = the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import iq_ref
from gnuais_amd import params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def dev(x, device=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")


def hard_pairs(rng, n_rows, n_ch):
    """full-range random pairs with rows of the values the definition singles out mixed in: +-32767, -32768, 0, equal
    magnitudes (|re| == |im|) and pairs whose products are -0.0"""
    x = rng.integers(-32768, 32768, (n_rows, n_ch, 2)).astype(np.int16)
    special = np.array([32767, -32767, -32768, 0, 1, -1, 5, -5], dtype=np.int16)
    m = rng.random((n_rows, n_ch)) < 0.3
    x[m] = rng.choice(special, (int(m.sum()), 2))
    t = rng.random((n_rows, n_ch)) < 0.1                 # (a, a) or (a, -a): ties against any real previous pair
    a = rng.choice(special, int(t.sum()))
    x[t] = np.stack([a, a * rng.choice(np.array([1, -1], dtype=np.int16), a.size)], axis=1)
    return x


@pytest.mark.parametrize("n_ch", [1, 3, 65, 1000, 4096])
def test_discriminate_bit_exact_ragged_carry_and_reset(n_ch):
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(100 + n_ch)
    chunks = [1, 63, 64, 65, 200, 1, 129] if n_ch <= 1000 else [1, 130, 64, 257]
    x = hard_pairs(rng, sum(chunks) * 2, n_ch)
    b = ReceiverBatch(n_ch, max_len=max(chunks))
    carry = None
    pos = 0
    for rep in range(2):
        for n in chunks:
            seg = x[pos:pos + n]
            pos += n
            got = b.discriminate(dev(seg)).cpu().numpy()
            want, carry = iq_ref.discriminate(seg, carry)
            assert got.dtype == np.int16 and got.shape == (n, n_ch)
            assert np.array_equal(got, want), (n_ch, rep, n, np.argwhere(got != want)[:5])
        b.reset()                                        # the carry is (0, 0) again
        carry = None
    assert pos == x.shape[0]


def test_discriminate_unaligned_views():
    """a view that starts one channel in (4-byte aligned pointers only): the narrow lane form; the same numbers"""
    from gnuais_amd import ReceiverBatch
    import torch
    rng = np.random.default_rng(9)
    n_ch = 64
    x = hard_pairs(rng, 300, n_ch + 1)
    whole = dev(x.reshape(-1)).view(torch.int16)
    part = whole[2:2 + 300 * n_ch * 2].view(300, n_ch, 2)      # not 16-byte aligned
    b = ReceiverBatch(n_ch, max_len=300)
    got = b.discriminate(part).cpu().numpy()
    want, _ = iq_ref.discriminate(part.cpu().numpy())
    assert np.array_equal(got, want)


def frames_state(b):
    cnt = b.counters()
    return (b.drain_frames().tobytes(), cnt.tobytes(), b.pll_state().tobytes(), b.fsm_state().tobytes(),
            b.maxval().tobytes())


def iq_streams(n_ch, total, sps=5, seed=3, sigmas=(0.0, 800.0, 1500.0, 3000.0)):
    made = [synth.make_iq_stream(total, seed=seed, channel=c, sps=sps, sigma=sigmas[c % len(sigmas)], occupancy=0.8)
            for c in range(n_ch)]
    return np.stack([m[0] for m in made], axis=1), [m[1] for m in made]


@pytest.mark.parametrize("rate", ["48k", "192k"])
def test_run_iq_equals_run_on_restated_audio_and_the_oracle(rate):
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    sps, kw = (5, {}) if rate == "48k" else (20, dict(taps=params.taps_192k(), pllinc=params.PLLINC_192K))
    n_ch = 37
    total = (24 if rate == "48k" else 8) * synth.SLOT_BITS * sps
    x, placed = iq_streams(n_ch, total, sps)
    chunks = [1020, 1, 4096, 333, 7000]
    chunks.append(total - sum(chunks))
    a = ReceiverBatch(n_ch, max_len=max(chunks), **kw)
    r = ReceiverBatch(n_ch, max_len=max(chunks), **kw)
    o = Oracle(n_ch, **kw)
    carry, pos = None, 0
    for n in chunks:                                     # pipelined: no sync between the calls
        seg = x[pos:pos + n]
        pos += n
        audio, carry = iq_ref.discriminate(seg, carry)
        a.run_iq(dev(seg), sync=False)
        r.run(dev(audio), sync=False)
        o.run(audio)
    a.sync()
    r.sync()
    got, want = frames_state(a), frames_state(r)
    assert got == want
    assert got[0] == o.frames().tobytes()
    cnt = a.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), o.counters())
    assert cnt["receivedframes"].sum() > (300 if rate == "48k" else 80)
    # the host form: copy, run, sync
    a.reset()
    r.reset()
    audio = iq_ref.discriminate(x)[0]
    pos = 0
    for n in chunks:
        a.run_iq(x[pos:pos + n])
        r.run(audio[pos:pos + n])
        pos += n
    assert frames_state(a)[:4] == frames_state(r)[:4]


def test_stream_change_between_run_iq_calls():
    """Each call on a stream of its own and nothing synchronised by the caller: the library drains the previous stream
    before the discriminator overwrites the audio the previous call's FIR reads."""
    import torch
    from gnuais_amd import ReceiverBatch
    n_ch, total = 512, 16 * 1280
    x, _ = iq_streams(n_ch, total)
    xd = dev(x)
    chunks = [4000] * 5
    chunks.append(total - sum(chunks))
    one = ReceiverBatch(n_ch, max_len=4000)
    many = ReceiverBatch(n_ch, max_len=4000)
    streams = [torch.cuda.Stream() for _ in range(3)]
    pos = 0
    for i, n in enumerate(chunks):
        one.run_iq(xd[pos:pos + n], sync=False)
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())      # the input exists before the side stream reads it
        with torch.cuda.stream(st):
            many.run_iq(xd[pos:pos + n], sync=False)
        pos += n
    one.sync()
    many.sync()
    torch.cuda.synchronize()
    assert frames_state(one) == frames_state(many)
    assert one.counters()["receivedframes"].sum() > 1000


def test_c3_shape_discriminate_and_run_iq():
    """16384 channels x 48000 samples, I/Q tiled from 256 base streams (as bench.py tiles audio)."""
    import torch
    from gnuais_amd import ReceiverBatch
    n_ch, total, k = 16384, 48000, 256
    base, _ = iq_streams(k, total, seed=77)                                  # [total][k][2]
    rot = np.array([synth.rotation_of(c, total) for c in range(n_ch)])
    bd = dev(base)
    rot = torch.from_numpy(rot).to(bd.device)
    cols = torch.arange(n_ch, device=bd.device) % k
    xd = torch.empty((total, n_ch, 2), dtype=torch.int16, device=bd.device)
    for lo in range(0, total, 4096):                                         # channel c = base c % k, rotated
        r = (torch.arange(lo, min(lo + 4096, total), device=bd.device)[:, None] + rot[None, :]) % total
        xd[lo:lo + r.shape[0]] = bd[r, cols[None, :]]
    b = ReceiverBatch(n_ch, max_len=total)
    audio = b.discriminate(xd)
    # the restatement on a band of rows across every channel (row 0 follows the (0, 0) carry, the band its row before)
    for lo, hi in ((0, 200), (23_950, 24_140), (total - 130, total)):
        seg = xd[max(lo - 1, 0):hi].cpu().numpy()
        want, _ = iq_ref.discriminate(seg[1:], seg[0]) if lo else iq_ref.discriminate(seg)
        assert np.array_equal(audio[lo:hi].cpu().numpy(), want), lo
    b.reset()
    r = ReceiverBatch(n_ch, max_len=total)
    b.run_iq(xd)
    r.run(audio)
    got, want = frames_state(b), frames_state(r)
    assert got == want
    assert b.counters()["receivedframes"].sum() > 100000


def test_node_run_iq_host_equals_one_batch():
    """gnuais_node_run_iq_host from one host array and, in a second pass, gnuais_node_run_iq from device slabs, against
    one batch"""
    from gnuais_amd import ReceiverBatch, ReceiverNode
    n_ch, total = 203, 10 * 1280
    x, _ = iq_streams(n_ch, total)
    nd = ReceiverNode(n_ch, devices=[0, 0, 0, 0], max_len=5000)
    b = ReceiverBatch(n_ch, max_len=5000)
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
        assert b.counters()["receivedframes"].sum() > 200
        nd.reset()
        b.reset()
    nd.close()


def test_decode_file_iq_equals_the_audio_path(tmp_path):
    from gnuais_amd import io
    x, _ = iq_streams(2, 20 * 1280, sigmas=(1000.0,))
    iq_path, au_path = str(tmp_path / "iq.wav"), str(tmp_path / "audio.wav")
    io.write_wav(iq_path, 48000, x.reshape(x.shape[0], 4))                  # 2 receivers = 4 channels: I0 Q0 I1 Q1
    io.write_wav(au_path, 48000, iq_ref.discriminate(x)[0])
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), *a, "--call", "5000"],
                                    check=True, capture_output=True, text=True, timeout=300)
    got, want = run(iq_path, "--iq"), run(au_path)
    assert got.stdout == want.stdout and got.stdout.count("!AIVDM") > 20
    raw = str(tmp_path / "iq.raw")
    x.tofile(raw)
    assert run(raw, "--raw", "4", "--iq").stdout == want.stdout
