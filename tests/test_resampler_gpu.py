"""Wideband in at a rational ratio on the device (gnuais_batch_resampler, resampler.hip): bit for bit against the NumPy
restatement on converted input, resample_ref.Resampler(...).run(convert(x)) (tests/resample_ref.py), over the matrix of
tests/resample_cases.py; formats mixed on one batch; alignment; a medium shape; resampler(1, 6) against channeliser(6);
and run_wideband end to end -- device, host and node forms, the AFC, frame times and their slots, stream changes, and
audio / I/Q / wideband calls mixed on one batch."""
import ctypes as C
import functools

import numpy as np
import pytest

import afc_ref
import chan_cases
import chan_ref
import frame_time_ref as ftr
import iq_ref
import resample_cases as cases
import resample_ref as rr
import wide_format_cases
from wide_format_ref import PAIR_BYTES, VALUE, convert, quantise
from gnuais_amd import synth

pytestmark = pytest.mark.gpu


def dev(x, device=0):
    import torch
    return torch.from_numpy(np.array(x)).to(f"cuda:{device}")             # a copy: the shared captures are read-only


def hard_input(rng, n, M, fmt):
    return chan_cases.hard_wide(rng, n, M) if fmt == "cs16" else wide_format_cases.hard_input(rng, n, M, fmt)


def configured(case, max_rows=None):
    from gnuais_amd import ReceiverBatch
    b = ReceiverBatch(case.M * case.K, max_len=max_rows or case.max_rows)
    b.resampler(case.up, case.down, case.rate, case.offsets, taps=case.taps if case.T else None)
    ref = rr.Resampler(case.M, case.up, case.down, case.rate, case.offsets, taps=case.taps)
    return b, ref


def run_case(case, fmt):
    rng = np.random.default_rng(case.up * 7919 + case.down * 31 + case.K + case.T + 100003 * VALUE[fmt])
    b, ref = configured(case)
    assert b.info("rows") == 0
    for p in case.periods:
        if p == 0:
            b.reset()
            ref.reset()
            continue
        n = p * case.down
        x = hard_input(rng, n, case.M, fmt)
        got = b.channelise(dev(x), fmt=None if fmt == "cs16" else fmt).cpu().numpy()
        want = ref.run(convert(x, fmt))
        assert got.shape == (p * case.up, case.M * case.K, 2)
        assert np.array_equal(got, want), (case.name, fmt, p, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_every_ratio_and_form_bit_exact_ragged_and_reset(case):
    run_case(case, "cs16")


@pytest.mark.parametrize("fmt,case", cases.FORMAT_CASES, ids=cases.FORMAT_IDS)
def test_every_format_bit_exact(fmt, case):
    run_case(case, fmt)


@pytest.mark.parametrize("up,down", [(3, 128), (2, 3)])
def test_formats_mixed_on_one_batch(up, down):
    """consecutive calls in every format, so that every call reads a carry that a call of another format wrote (calls
    shorter than the carry among them): the concatenated output is one restatement run over the converted parts"""
    case = cases.Case("mixed", up, down, 3, 2, (50,))
    b, ref = configured(case)
    rng = np.random.default_rng(down)
    order = ["cs16", "cu8", "cf32", "cs8", "cu8", "cs16", "cs8", "cf32"]
    periods = [7, 1, 50, 1, 44, 1, 2, 9]
    outs, parts = [], []
    for i, (fmt, p) in enumerate(zip(order, periods)):
        x = hard_input(rng, p * down, case.M, fmt)
        parts.append(convert(x, fmt))
        outs.append(b.channelise(dev(x), fmt=None if i == 0 else fmt).cpu().numpy())
    whole = ref.run(np.concatenate(parts))
    got = np.concatenate(outs)
    assert np.array_equal(got, whole), np.argwhere(got != whole)[:5]


def raw_channelise_fmt(b, fmt, in_ptr, n, out_ptr):
    import torch
    s = torch.cuda.current_stream()
    rc = b._lib.gnuais_batch_channelise_fmt(b._h, VALUE[fmt], C.c_void_p(in_ptr), int(n), C.c_void_p(out_ptr),
                                            C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc


@pytest.mark.parametrize("fmt,good,bad", [("cs16", (4, 8, 12), (2,)), ("cu8", (2, 6, 14), (1, 7)), ("cs8", (2, 10), (3,)),
                                          ("cf32", (4, 12), (2, 6))])
def test_input_at_every_allowed_alignment(fmt, good, bad):
    """input at every allowed offset past a 16-byte boundary is accepted and exact; off the format's alignment it is
    refused and the state stays untouched"""
    import torch
    from gnuais_amd import lib
    case = cases.Case("align", 3, 64, 3, 3, (6,))
    b, ref = configured(case)
    rng = np.random.default_rng(5)
    for i, p in enumerate([1, 6, 2, 5]):
        n = p * case.down
        x = hard_input(rng, n, case.M, fmt)
        nbytes = n * case.M * PAIR_BYTES[fmt]
        buf = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        out = torch.empty((p * case.up, case.M * case.K, 2), dtype=torch.int16, device="cuda:0")
        raw = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
        for off in bad:
            buf[off:off + nbytes] = raw
            assert raw_channelise_fmt(b, fmt, buf.data_ptr() + off, n, out.data_ptr()) == lib.E_ARG
            assert "aligned" in b._lib.gnuais_last_error().decode()
        off = good[i % len(good)]
        buf[off:off + nbytes] = raw
        assert raw_channelise_fmt(b, fmt, buf.data_ptr() + off, n, out.data_ptr()) == lib.OK
        want = ref.run(convert(x, fmt))
        assert np.array_equal(out.cpu().numpy(), want), (fmt, i, off)


def test_unaligned_output_takes_the_direct_form():
    """K = 2 stores 8 bytes per lane: an output 4 bytes off takes the direct form and gives the same rows"""
    import torch
    from gnuais_amd import lib
    case = cases.Case("out", 3, 64, 3, 2, (6,))
    b, ref = configured(case)
    x = chan_cases.hard_wide(np.random.default_rng(1), 6 * 64, 3)
    buf = torch.zeros(18 * 6 * 4 + 16, dtype=torch.uint8, device="cuda:0")
    assert raw_channelise_fmt(b, "cs16", dev(x).data_ptr(), 6 * 64, buf.data_ptr() + 2) == lib.E_ARG
    xd = dev(x)
    assert raw_channelise_fmt(b, "cs16", xd.data_ptr(), 6 * 64, buf.data_ptr() + 4) == lib.OK
    got = buf[4:4 + 18 * 6 * 4].cpu().numpy().view(np.int16).reshape(18, 6, 2)
    assert np.array_equal(got, ref.run(x))


def test_bad_configurations_and_calls_are_refused():
    from gnuais_amd import ReceiverBatch, lib
    b = ReceiverBatch(4, max_len=30)
    offs = [-25000, 25000]
    for up, down in ((6, 128), (3, 3), (6, 5), (3, 1025), (0, 5), (65, 128)):
        with pytest.raises(lib.GnuaisError) as e:
            b.resampler(up, down, 2048000, offs)
        assert e.value.code == lib.E_ARG
    with pytest.raises(lib.GnuaisError, match="65535"):
        b.resampler(2, 3, 72000, offs, taps=[32767, 1, 32767, 32767, 2])
    b.resampler(2, 3, 72000, offs, taps=[32767, 1, 32767, 32767, 1])
    with pytest.raises(lib.GnuaisError, match="n_taps"):
        b.resampler(2, 3, 72000, offs, taps=np.zeros(16386, dtype=np.int16))
    with pytest.raises(lib.GnuaisError, match="multiple of n_offsets"):
        b.resampler(3, 128, 2048000, [1, 2, 3])
    b.resampler(3, 128, 2048000, offs)
    x = dev(np.zeros((11 * 128, 2, 2), dtype=np.int16))
    out = dev(np.zeros((33, 4, 2), dtype=np.int16))
    for n in (127, 129, 0, 11 * 128):                               # not a multiple of D; 33 rows > max_len
        rc = b._lib.gnuais_batch_channelise(b._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None)
        assert rc == lib.E_ARG and "down = 128" in b._lib.gnuais_last_error().decode(), n
        rc = b._lib.gnuais_batch_run_wideband(b._h, C.c_void_p(x.data_ptr()), n, None)
        assert rc == lib.E_ARG
    assert b.channelise(x[:10 * 128]).shape == (30, 4, 2)
    # the integer map cannot describe a ratio: it says so and names the call that can
    with pytest.raises(lib.GnuaisError, match="gnuais_batch_time_map_ratio") as e:
        b.time_map("wideband")
    assert e.value.code == lib.E_STATE
    assert b.time_map_ratio("wideband") == rr.time_map_ratio(3, 128, 2049)
    assert b.time_map_ratio("audio") == (1, 1, -18) and b.time_map_ratio("iq") == (1, 1, -18)


def test_medium_shape_every_receiver():
    """256 streams x 2 offsets at 3/128, one call of 400 periods (1200 rows: ten segments, four stream groups)"""
    case = cases.Case("medium", 3, 128, 256, 2, (400,))
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(11)
    x = chan_cases.hard_wide(rng, 400 * 128, 256)
    b = ReceiverBatch(512, max_len=1200)
    b.resampler(3, 128, case.rate, case.offsets)
    got = b.channelise(dev(x)).cpu().numpy()
    assert got.shape == (1200, 512, 2)
    for s0 in range(0, 256, 32):                                     # the restatement in stream chunks, to bound memory
        want = rr.Resampler(32, 3, 128, case.rate, case.offsets).run(x[:, s0:s0 + 32])
        assert np.array_equal(got[:, 2 * s0:2 * s0 + 64], want), (s0, np.argwhere(got[:, 2 * s0:2 * s0 + 64] != want)[:5])


def test_resampler_1_6_is_channeliser_6():
    """up = 1, down <= 64 configures what channeliser(down) configures: the same outputs over ragged calls (each reads
    the carry the one before wrote), the same time map, the channeliser's own limits and messages"""
    from gnuais_amd import ReceiverBatch, lib
    M, K, D = 65, 2, 6
    rng = np.random.default_rng(6)
    calls = [1, 37, 300, 2, 129]
    a, b = ReceiverBatch(M * K, max_len=300), ReceiverBatch(M * K, max_len=300)
    a.channeliser(D, 288000, cases.OFFS[K])
    b.resampler(1, D, 288000, cases.OFFS[K])
    ref = chan_ref.Channeliser(M, D, 288000, cases.OFFS[K])
    for r in calls:
        x = dev(chan_cases.hard_wide(rng, r * D, M))
        ga, gb = a.channelise(x).cpu().numpy(), b.channelise(x).cpu().numpy()
        assert np.array_equal(ga, gb) and np.array_equal(gb, ref.run(x.cpu().numpy()))
    assert a.time_map("wideband") == b.time_map("wideband")
    assert b.time_map_ratio("wideband") == (6, 1, b.time_map("wideband")[1])
    with pytest.raises(lib.GnuaisError, match="channeliser: n_taps must be 1..1025"):
        b.resampler(1, D, 288000, cases.OFFS[K], taps=np.ones(1026, dtype=np.int16))
    # channeliser_for_rate picks between the two
    assert b.channeliser_for_rate(288000, cases.OFFS[K]) == (1, 6) and b.time_map("wideband")[0] == 6
    assert b.channeliser_for_rate(2048000, cases.OFFS[K]) == (3, 128) and b.time_map_ratio("wideband")[:2] == (128, 3)
    assert b.channeliser_for_rate(250000, cases.OFFS[K]) == (24, 125)
    # U = 1 with D > 64 is the rational form's
    c = ReceiverBatch(2, max_len=8)
    c.resampler(1, 125, 6000000, cases.OFFS[K])
    x = chan_cases.hard_wide(rng, 8 * 125, 1)
    assert np.array_equal(c.channelise(dev(x)).cpu().numpy(), rr.Resampler(1, 1, 125, 6000000, cases.OFFS[K]).run(x))


# ---- end to end ----

def frames_state(b):
    cnt = b.counters()
    return (b.drain_frames().tobytes(), cnt.tobytes(), b.pll_state().tobytes(), b.fsm_state().tobytes(), b.maxval().tobytes())


@functools.lru_cache(maxsize=4)
def capture(up, down, M, W, slots=12):
    """M streams of the CPU decode test's capture (gated, with a carrier error where the AFC is on), read-only"""
    n = slots * 1280 * down // up
    assert n % down == 0
    made = [synth.make_resampled_wideband_stream(n, up, down, (-25000, 25000), seed=5, stream=s, sigma=300.0, occupancy=0.7,
                                                 gated=True, offset_hz=2500.0 if W else 0.0) for s in range(M)]
    x = np.stack([m[0] for m in made], axis=1)
    x.flags.writeable = False
    return x, [p for m in made for p in m[1]]


@pytest.mark.parametrize("W", [0, 1024])
@pytest.mark.parametrize("up,down", [(3, 128), (24, 125)])
def test_run_wideband_end_to_end_device_host_node_times_and_slots(up, down, W):
    """run_wideband on device input with frame times, on host input and on a node of two shards, over ragged calls:
    frames and counters equal the oracle's on resample_ref -> iq_ref (-> afc_ref), the times equal frame_time_ref's,
    and every frame's input index (t * num + off) // den lies in the slot its payload was placed in"""
    from gnuais_amd import ReceiverBatch, ReceiverNode
    M, K, offs = 2, 2, [-25000, 25000]
    N, rate = M * K, 48000 * down // up
    x, placed = capture(up, down, M, W)
    periods = x.shape[0] // down
    cuts = [0, 1, periods // 8, periods // 8 + 1, periods // 3, periods]
    rows = max(b - a for a, b in zip(cuts[:-1], cuts[1:])) * up
    d, h = ReceiverBatch(N, max_len=rows), ReceiverBatch(N, max_len=rows)
    nd = ReceiverNode(N, devices=[0, 0], max_len=rows)
    for b in (d, h, nd):
        b.resampler(up, down, rate, offs)
        if W:
            b.afc(W)
    d.frame_times(True)
    r, afc, carry, ref = rr.Resampler(M, up, down, rate, offs), (afc_ref.Afc(N, W) if W else None), None, ftr.FrameTimeRef(N)
    num, den, off = d.time_map_ratio("wideband")
    assert (num, den, off) == rr.time_map_ratio(up, down, 16 * down + 1, afc_window=W)
    frames, checked = [], 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        seg = x[a * down:e * down]
        d.run_wideband(dev(seg), sync=False)
        h.run_wideband(seg)
        nd.run_wideband_host(seg)
        iq = r.run(seg)
        if afc:
            audio = afc.apply(iq)
        else:
            audio, carry = iq_ref.discriminate(iq, carry)
        ref.run(audio)
        fr, t = d.drain_frames_timed()
        wf, wt = ref.drain()
        assert fr.tobytes() == wf.tobytes(), (len(fr), len(wf))
        assert np.array_equal(t, wt)
        for f, ti in zip(fr, t):
            index = (int(ti) * num + off) // den
            slot = (index * up) // (1280 * down)
            want = dict(placed[int(f["channel"])]).get(slot)
            assert want is not None and bytes(f["payload"][: int(f["nbits"]) // 8]) == want, (int(f["channel"]), int(ti), slot)
            checked += 1
        frames.append(fr)
    assert checked > 10
    cnt = d.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), ref.o.counters())
    nd.sync()
    hf = h.drain_frames()
    # the per-call drains of d, concatenated and put in one drain's order (channel, then end_bit), are h's one drain
    allf = np.concatenate(frames)
    order = np.lexsort((ftr.stamp(allf), allf["channel"]))
    assert hf.tobytes() == allf[order].tobytes()
    assert h.counters().tobytes() == cnt.tobytes()
    assert nd.drain_frames().tobytes() == hf.tobytes() and nd.counters().tobytes() == cnt.tobytes()
    assert nd.time_map_ratio("wideband") == (num, den, off)
    nd.close()


def test_stream_change_between_calls():
    """the drain rule for the rational form: every call on another stream, nothing synchronised by the caller,
    against the same calls on one stream"""
    import torch
    from gnuais_amd import ReceiverBatch
    up, down, M = 3, 128, 2
    x, _ = capture(up, down, M, 0)
    periods = x.shape[0] // down
    cuts = [0, 850, 1700, 2550, 3400, 4250, periods]
    assert periods == 5120
    one, many = ReceiverBatch(2 * M, max_len=870 * up), ReceiverBatch(2 * M, max_len=870 * up)
    for b in (one, many):
        b.resampler(up, down, 2048000, [-25000, 25000])
    streams = [torch.cuda.Stream() for _ in range(3)]
    parts = [dev(x[a * down:e * down]) for a, e in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    for i, xd in enumerate(parts):
        one.run_wideband(xd, sync=False)
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            many.run_wideband(xd, sync=False)
    one.sync()
    many.sync()
    torch.cuda.synchronize()
    assert frames_state(one) == frames_state(many)
    assert one.counters()["receivedframes"].sum() > 10


def test_audio_iq_and_wideband_calls_mixed_on_one_batch():
    """a wideband call at 3/128, an I/Q call, an audio call and a wideband call again: each form keeps its own carry,
    the chain sees the concatenated audio -- frames and counters equal the oracle's on that audio"""
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    up, down, M, N = 3, 128, 2, 4
    x, _ = capture(up, down, M, 0)
    half = (x.shape[0] // down // 2) * down
    iq_in = np.stack([synth.make_iq_stream(3 * 1280, seed=2, channel=c, sigma=800.0, occupancy=0.8)[0] for c in range(N)], axis=1)
    au_in = np.stack([synth.make_stream(3 * 1280, seed=2, channel=c, occupancy=0.8)[0] for c in range(N)], axis=1)
    b = ReceiverBatch(N, max_len=half // down * up)
    b.resampler(up, down, 2048000, [-25000, 25000])
    r = rr.Resampler(M, up, down, 2048000, [-25000, 25000])
    b.run_wideband(dev(x[:half]), sync=False)
    a1, carry = iq_ref.discriminate(r.run(x[:half]))
    b.run_iq(dev(iq_in), sync=False)
    a2, carry = iq_ref.discriminate(iq_in, carry)
    b.run(dev(au_in), sync=False)
    b.run_wideband(dev(x[half:]), sync=False)
    a3, carry = iq_ref.discriminate(r.run(x[half:]), carry)
    b.sync()
    o = Oracle(N)
    o.run(np.concatenate([a1, a2, au_in, a3]))
    want = o.frames()
    assert len(want) > 10
    assert b.drain_frames().tobytes() == want.tobytes()
    cnt = b.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), o.counters())


def test_decode_file_wideband_auto_equals_the_iq_path(tmp_path):
    """decode_file.py --wideband auto --rate 2048000 on a cs16 capture whose length is no multiple of D (the tail is
    trimmed) prints what --iq prints on the restatement's narrowband I/Q; --times tags every sentence through the ratio
    map, and the sentences behind the tags are the same"""
    import os
    import re
    import subprocess
    import sys
    from gnuais_amd import io
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    up, down, M = 3, 128, 2
    x, _ = capture(up, down, M, 0)
    iq = rr.Resampler(M, up, down, 2048000, [-25000, 25000]).run(x)
    wide_path, iq_path = str(tmp_path / "wide.cs16"), str(tmp_path / "iq.wav")
    np.concatenate([x, x[:77]]).tofile(wide_path)                     # 77 samples past the last whole period
    io.write_wav(iq_path, 48000, iq.reshape(iq.shape[0], 4 * M))
    # --call 4998 = 1666 periods of 3 rows: both runs cut the rows alike
    run = lambda *a: subprocess.run([sys.executable, os.path.join(root, "scripts", "decode_file.py"), *a, "--call", "4998"],
                                    check=True, capture_output=True, text=True, timeout=300)
    auto = (wide_path, "--wideband", "auto", "--rate", "2048000", "--streams", str(M))
    got, want = run(*auto), run(iq_path, "--iq")
    assert got.stdout == want.stdout and got.stdout.count("!AIVDM") > 10
    tagged = run(*auto, "--times", "--start", "1000").stdout
    assert re.sub(r"\\c:\d+\*[0-9A-F]{2}\\", "", tagged) == got.stdout
    secs = [int(v) for v in re.findall(r"\\c:(\d+)\*", tagged)]
    assert len(secs) == got.stdout.count("!AIVDM") and min(secs) >= 1000 and max(secs) <= 1000 + x.shape[0] // 2048000
    bad = subprocess.run([sys.executable, os.path.join(root, "scripts", "decode_file.py"), wide_path, "--wideband", "auto",
                          "--rate", "2048001"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "outside" in bad.stderr
