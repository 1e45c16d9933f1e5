"""Sample formats of wideband input on the device (gnuais_batch_channelise_fmt / _run_wideband_fmt, channeliser_fmt.hip):
cu8, cs8 and cf32 captures converted where the channeliser loads them, bit for bit against the NumPy restatement on
converted input, chan_ref.Channeliser(...).run(convert(x)) (tests/chan_ref.py, tests/wide_format_ref.py), over the
matrix of tests/wide_format_cases.py; formats mixed on one batch; alignment; run_wideband end to end with its host and
node forms and the AFC; the W3 shape in cu8; decode_file.py --format; and the drain rule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import chan_cases
import chan_ref
import iq_ref
import wide_format_cases as cases
from wide_format_ref import DTYPE, PAIR_BYTES, VALUE, convert, quantise
from gnuais_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x, device=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")


def configure(case, b):
    b.channeliser(case.D, case.R, list(case.offsets), taps=None if case.taps_kind == "default" else case.taps)


@pytest.mark.parametrize("fmt,case", cases.CASES, ids=cases.CASE_IDS)
def test_every_form_of_every_format_bit_exact_ragged_and_reset(fmt, case):
    """the calls of test_channeliser_forms_gpu.test_every_form_bit_exact_ragged_and_reset on input of format fmt"""
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(case.K * 7919 + case.D * 31 + case.T + 100003 * VALUE[fmt])
    chunks = case.chunks
    x = cases.hard_input(rng, sum(chunks), case.M, fmt)
    v = convert(x, fmt)
    b = ReceiverBatch(case.M * case.K, max_len=max(case.rows))
    configure(case, b)
    ref = chan_ref.Channeliser(case.M, case.D, case.R, case.offsets, taps=case.taps)
    for rep, calls in enumerate((chunks, chunks[:2])):
        pos = 0
        for n in calls:
            got = b.channelise(dev(x[pos:pos + n]), fmt=fmt).cpu().numpy()
            want = ref.run(v[pos:pos + n])
            pos += n
            assert got.shape == (n // case.D, case.M * case.K, 2)
            assert np.array_equal(got, want), (fmt, case.name, rep, n, np.argwhere(got != want)[:5])
        b.reset()
        ref.reset()


@pytest.mark.parametrize("name", ["k2_na17_T1025", "k3_na17_bottom", "k5_direct", "k1_na4_T1"])
def test_formats_mixed_on_one_batch(name):
    """consecutive calls in cs16, cu8, cf32, cs8 and cu8 again, so that every call reads a carry that a call of another
    format wrote (1-row calls shorter than T-1 among them): the concatenated output is one chan_ref run over the
    concatenation of the converted parts; the fmt-less entry and fmt="cs16" are the same call"""
    from gnuais_amd import ReceiverBatch
    case = {c.name: c for c in chan_cases.CASES}[name]
    rng = np.random.default_rng(case.T)
    order = ["cs16", "cu8", "cf32", "cs8", "cu8", "cs16", "cs8", "cf32"]
    rows = [37, 1, 300, 1, 129, 1, 2, 40]
    b = ReceiverBatch(case.M * case.K, max_len=max(rows))
    configure(case, b)
    outs, parts = [], []
    for i, (fmt, r) in enumerate(zip(order, rows)):
        n = r * case.D
        x = chan_cases.hard_wide(rng, n, case.M) if fmt == "cs16" else cases.hard_input(rng, n, case.M, fmt)
        parts.append(convert(x, fmt))
        outs.append(b.channelise(dev(x), fmt=None if i == 0 else fmt).cpu().numpy())
    whole = chan_ref.Channeliser(case.M, case.D, case.R, case.offsets, taps=case.taps).run(np.concatenate(parts))
    got = np.concatenate(outs)
    assert np.array_equal(got, whole), (name, np.argwhere(got != whole)[:5])


def raw_channelise_fmt(b, fmt, in_ptr, n, out_ptr):
    """gnuais_batch_channelise_fmt on raw addresses, on torch's current stream; returns the status"""
    import torch
    s = torch.cuda.current_stream()
    rc = b._lib.gnuais_batch_channelise_fmt(b._h, VALUE[fmt], C.c_void_p(in_ptr), int(n), C.c_void_p(out_ptr),
                                            C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc


@pytest.mark.parametrize("fmt,good,bad", [("cu8", (2, 6, 14), (1, 7)), ("cs8", (2, 10), (3,)), ("cf32", (4, 12), (2, 6))])
def test_input_alignment_per_format(fmt, good, bad):
    """cu8 / cs8 input 2, 6, 14 bytes past a 16-byte boundary is accepted and exact, at an odd address refused; cf32 at
    4 and 12 accepted, at 2 refused; a refused call names the format and leaves the state untouched"""
    import torch
    from gnuais_amd import ReceiverBatch, lib
    case = {c.name: c for c in chan_cases.CASES}["k3_na17_bottom"]
    rng = np.random.default_rng(17)
    calls = [case.D * r for r in (37, 1, 300, 2, 129)]
    x = cases.hard_input(rng, sum(calls), case.M, fmt)
    b = ReceiverBatch(case.M * case.K, max_len=300)
    configure(case, b)
    ref = chan_ref.Channeliser(case.M, case.D, case.R, case.offsets, taps=case.taps)
    pos = 0
    for i, n in enumerate(calls):
        nbytes = n * case.M * PAIR_BYTES[fmt]
        buf = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        out = torch.empty((n // case.D, case.M * case.K, 2), dtype=torch.int16, device="cuda:0")
        raw = torch.from_numpy(np.ascontiguousarray(x[pos:pos + n]).view(np.uint8).reshape(-1)).cuda()
        for off in bad:
            buf[off:off + nbytes] = raw
            assert raw_channelise_fmt(b, fmt, buf.data_ptr() + off, n, out.data_ptr()) == lib.E_ARG
            msg = b._lib.gnuais_last_error().decode()
            assert fmt in msg and "aligned" in msg, msg
        off = good[i % len(good)]
        buf[off:off + nbytes] = raw
        assert raw_channelise_fmt(b, fmt, buf.data_ptr() + off, n, out.data_ptr()) == lib.OK
        want = ref.run(convert(x[pos:pos + n], fmt))     # the refused calls did not advance the carry or n
        assert np.array_equal(out.cpu().numpy(), want), (fmt, i, off)
        pos += n
    assert raw_channelise_fmt(b, "cu8", 0, calls[0], out.data_ptr()) == lib.E_ARG
    rc = b._lib.gnuais_batch_channelise_fmt(b._h, 4, C.c_void_p(buf.data_ptr()), calls[1], C.c_void_p(out.data_ptr()), None)
    assert rc == lib.E_ARG and "format" in b._lib.gnuais_last_error().decode()


@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("K,D,shifts", [(2, 3, (4, 8, 12, 0, 4)), (4, 2, (8, 16, 4, 12, 0))])
def test_unaligned_output_takes_the_direct_form_for_every_format(fmt, K, D, shifts):
    """as test_channeliser_forms_gpu.test_unaligned_output_falls_back_to_the_direct_form: an output off the fast form's
    vector store takes the format's direct kernel; calls alternate between the forms on one batch"""
    import torch
    from gnuais_amd import ReceiverBatch, lib
    M = 65
    rows_per_call = (37, 1, 300, 2, 129)
    N = M * K
    rng = np.random.default_rng(K + 10 * VALUE[fmt])
    x = cases.hard_input(rng, D * sum(rows_per_call), M, fmt)
    b = ReceiverBatch(N, max_len=max(rows_per_call))
    offs = [-25000, 25000, 12345, -7][:K]
    b.channeliser(D, 48000 * D, offs)
    assert chan_ref.fast_na(K, 16 * D + 1, D) == 17
    ref = chan_ref.Channeliser(M, D, 48000 * D, offs)
    fill = 0x5a5a
    pos = 0
    for rows, shift in zip(rows_per_call, shifts):
        n_words = rows * N
        buf = torch.full((2 * n_words + 64,), fill, dtype=torch.int16, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        xd = dev(x[pos:pos + rows * D])
        if rows == 1:                                   # refused: 2-byte aligned
            assert raw_channelise_fmt(b, fmt, xd.data_ptr(), rows * D, buf.data_ptr() + 2) == lib.E_ARG
            assert bool((buf == fill).all())
        assert raw_channelise_fmt(b, fmt, xd.data_ptr(), rows * D, buf.data_ptr() + shift) == lib.OK
        got = buf.cpu().numpy()
        e0, e1 = shift // 2, shift // 2 + 2 * n_words
        assert (got[:e0] == fill).all() and (got[e1:] == fill).all(), shift
        want = ref.run(convert(x[pos:pos + rows * D], fmt))
        pos += rows * D
        assert np.array_equal(got[e0:e1].reshape(want.shape), want), (fmt, K, shift, rows)


def test_python_fmt_takes_the_formats_dtype_only():
    """no silent casts: with fmt the array or tensor must have the format's dtype (complex64 [len][M] as well for
    cf32); fmt=None keeps casting NumPy input to int16 as before"""
    from gnuais_amd import ReceiverBatch
    M, D = 3, 2
    b = ReceiverBatch(2 * M, max_len=50)
    b.channeliser(D, 96000, [-25000, 25000])
    ref = chan_ref.Channeliser(M, D, 96000, [-25000, 25000])
    rng = np.random.default_rng(2)
    x = cases.hard_input(rng, 20, M, "cf32")
    for wrong in (np.zeros(x.shape, dtype=np.float64), convert(x, "cf32"), np.zeros(x.shape, dtype=np.uint8)):
        with pytest.raises(TypeError):
            b.channelise(wrong, fmt="cf32")
        with pytest.raises(TypeError):
            b.run_wideband(dev(wrong), fmt="cf32")
    with pytest.raises(TypeError):
        b.run_wideband(x, fmt="cu8")
    with pytest.raises(ValueError):
        b.run_wideband(x, fmt="cs32")
    z = x.view(np.complex64).reshape(x.shape[:2])               # the same bytes (arithmetic would quiet the NaNs)
    assert z.dtype == np.complex64 and z.tobytes() == x.tobytes()
    got = [b.channelise(x, fmt="cf32").cpu().numpy(), b.channelise(z, fmt="cf32").cpu().numpy(),
           b.channelise(dev(z), fmt="cf32").cpu().numpy()]
    v = convert(x, "cf32")
    for g in got:
        assert np.array_equal(g, ref.run(v))
    y = rng.integers(-3000, 3000, (20, M, 2))                   # int64: fmt=None casts, as it always did
    assert np.array_equal(b.channelise(y).cpu().numpy(), ref.run(y.astype(np.int16)))


def frames_state(b):
    cnt = b.counters()
    return (b.drain_frames().tobytes(), cnt.tobytes(), b.pll_state().tobytes(), b.fsm_state().tobytes(),
            b.maxval().tobytes())


def weak_capture(streams=4, slots=40, **kw):
    """the capture of the CPU decode test: amplitude 1500, sigma 225 at D = 6, both AIS offsets"""
    D, R, offs = 6, 288000, [-25000, 25000]
    n = slots * synth.SLOT_BITS * 5 * D
    made = [synth.make_wideband_stream(n, D, R, offs, seed=9, stream=s, amplitude=1500.0, sigma=225.0, occupancy=0.8, **kw)
            for s in range(streams)]
    return np.stack([m[0] for m in made], axis=1), [m[1] for m in made], D, R, offs


@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_run_wideband_fmt_end_to_end_host_and_node(fmt):
    """run_wideband(fmt) over ragged calls against run_wideband on convert(x) on a second batch (frames, counters, PLL
    and FSM state, maxval) and against the CPU oracle; at least 0.95 of the frames placed are decoded; the host form
    and the node form with two shards give the same frames"""
    from gnuais_amd import ReceiverBatch, ReceiverNode
    from oracle_lib import Oracle
    x16, placed, D, R, offs = weak_capture()
    M, K = x16.shape[1], len(offs)
    N, n = M * K, x16.shape[0]
    x = quantise(x16, fmt)
    v = convert(x, fmt)
    chunks = [D * 1020, D, D * 4096, D * 333]
    chunks.append(n - sum(chunks))
    rows = max(chunks) // D
    a, r, h = (ReceiverBatch(N, max_len=rows) for _ in range(3))
    nd = ReceiverNode(N, devices=[0, 0], max_len=rows)
    for b in (a, r, h, nd):
        b.channeliser(D, R, offs)
    pos = 0
    for c in chunks:
        a.run_wideband(dev(x[pos:pos + c]), sync=False, fmt=fmt)
        r.run_wideband(dev(v[pos:pos + c]), sync=False)
        h.run_wideband(x[pos:pos + c], fmt=fmt)                  # gnuais_batch_run_wideband_fmt_host: native bytes
        nd.run_wideband_fmt_host(x[pos:pos + c], fmt)
        pos += c
    a.sync()
    r.sync()
    nd.sync()
    got, want = frames_state(a), frames_state(r)
    assert got == want
    assert frames_state(h) == want
    assert nd.drain_frames().tobytes() == want[0] and nd.counters().tobytes() == want[1]
    nd.close()
    audio, _ = iq_ref.discriminate(chan_ref.Channeliser(M, D, R, offs).run(v))
    o = Oracle(N)
    o.run(audio)
    assert got[0] == o.frames().tobytes()
    cnt = a.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), o.counters())
    n_placed = sum(len(p) for m in placed for p in m)
    assert n_placed > 200 and cnt["receivedframes"].sum() >= 0.95 * n_placed, (cnt["receivedframes"].sum(), n_placed)


def test_cu8_with_afc_equals_cs16_on_converted_input():
    """afc(2048) and a 3 kHz carrier error: the cu8 calls give what the cs16 calls give on the converted samples"""
    from gnuais_amd import ReceiverBatch
    x16, placed, D, R, offs = weak_capture(offset_hz=3000.0, gated=True)
    M, N, n = x16.shape[1], x16.shape[1] * len(offs), x16.shape[0]
    x = quantise(x16, "cu8")
    v = convert(x, "cu8")
    chunks = [D * 1020, D, D * 4096, D * 333]
    chunks.append(n - sum(chunks))
    a, r = (ReceiverBatch(N, max_len=max(chunks) // D) for _ in range(2))
    for b in (a, r):
        b.channeliser(D, R, offs)
        b.afc(2048)
    pos = 0
    for c in chunks:
        a.run_wideband(dev(x[pos:pos + c]), sync=False, fmt="cu8")
        r.run_wideband(dev(v[pos:pos + c]), sync=False)
        pos += c
    a.sync()
    r.sync()
    assert np.array_equal(a.afc_estimate(), r.afc_estimate())
    got = frames_state(a)
    assert got == frames_state(r)
    assert a.counters()["receivedframes"].sum() > 0              # the comparison is not one of two empty results


def test_stream_change_between_run_wideband_fmt_calls():
    """the drain rule for the _fmt entries: every call on another stream, nothing synchronised by the
    caller, against the same calls on one stream; the shape of test_stream_change_between_run_wideband_calls"""
    import torch
    from gnuais_amd import ReceiverBatch
    M, D = 128, 6
    n = 12 * 1280 * D
    made = [synth.make_wideband_stream(n, D, 48000 * D, (-25000, 25000), seed=3, stream=s, sigma=800.0, occupancy=0.8)
            for s in range(M)]
    x16 = np.stack([m[0] for m in made], axis=1)
    fmts = ["cu8", "cf32", "cs8", "cs16", "cu8", "cf32"]
    chunks = [D * 3000] * 5
    chunks.append(n - sum(chunks))
    one = ReceiverBatch(2 * M, max_len=3000)
    many = ReceiverBatch(2 * M, max_len=3000)
    for b in (one, many):
        b.channeliser(D, 48000 * D, [-25000, 25000])
    streams = [torch.cuda.Stream() for _ in range(3)]
    pos = 0
    parts = []
    for fmt, c in zip(fmts, chunks):
        parts.append(dev(quantise(x16[pos:pos + c], fmt)))
        pos += c
    torch.cuda.synchronize()
    for i, (fmt, xd) in enumerate(zip(fmts, parts)):
        one.run_wideband(xd, sync=False, fmt=fmt)
        st = streams[i % 3]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            many.run_wideband(xd, sync=False, fmt=fmt)
    one.sync()
    many.sync()
    torch.cuda.synchronize()
    assert frames_state(one) == frames_state(many)
    assert one.counters()["receivedframes"].sum() > 1000


def torch_convert_cu8(xd):
    """the cu8 conversion in torch integer operations on the device: v = 256 u - 32640"""
    import torch
    out = torch.empty(xd.shape, dtype=torch.int16, device=xd.device)
    for lo in range(0, xd.shape[0], 16384):
        out[lo:lo + 16384] = (xd[lo:lo + 16384].to(torch.int32) * 256 - 32640).to(torch.int16)
    return out


def test_w3_shape_in_one_call_cu8():
    """8192 streams x K = 2 x D = 6, 288 000 wide samples of cu8 in one call (4.7 GB of input): all 16 384 receivers
    against chan_ref.torch_channelise on the tensor converted in torch integer operations, and 16 sampled streams
    against the NumPy restatement; the shape of test_channeliser_gpu.test_w3_shape_in_one_call"""
    import torch
    from gnuais_amd import ReceiverBatch
    M, K, D, n = 8192, 2, 6, 288000
    need = n * M * 2 * (1 + 2) + 2 * (n // D) * M * K * 4 + (16 << 30)     # input, its int16 copy, two outputs, int64 chunks
    free, _ = torch.cuda.mem_get_info(0)
    assert free >= need, f"the W3 check needs {need / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB are free"
    g = torch.Generator(device="cuda:0").manual_seed(11)
    xd = torch.randint(0, 256, (n, M, 2), dtype=torch.uint8, device="cuda:0", generator=g)
    b = ReceiverBatch(M * K, max_len=n // D)
    b.channeliser(D, 48000 * D, [-25000, 25000])
    out = b.channelise(xd, fmt="cu8")
    assert tuple(out.shape) == (n // D, M * K, 2)
    pick = np.random.default_rng(0).choice(M, 16, replace=False)
    pick.sort()
    sub = xd[:, torch.from_numpy(pick).to(xd.device)].cpu().numpy()
    want = chan_ref.Channeliser(16, D, 48000 * D, [-25000, 25000]).run(convert(sub, "cu8"))
    cols = (pick[:, None] * K + np.arange(K)[None, :]).reshape(-1)
    got = out[:, torch.from_numpy(cols).to(out.device)].cpu().numpy()
    assert np.array_equal(got, want)
    del got, sub
    vd = torch_convert_cu8(xd)
    del xd
    full = chan_ref.torch_channelise(vd, D, 48000 * D, [-25000, 25000], chan_ref.default_taps(D), chunk=512)
    assert full.shape == out.shape
    bad = int((full != out).sum())
    del full, out, vd
    torch.cuda.empty_cache()
    assert bad == 0, bad


def test_decode_file_format_cu8_prints_what_the_int16_path_prints(tmp_path):
    """decode_file.py --wideband 6 --rate 288000 on a .cu8 file (format from the extension, and named) against the
    int16 path on the converted samples"""
    x16, placed, D, R, offs = weak_capture(streams=2, slots=10)
    x = quantise(x16, "cu8")
    cu8_path, i16_path, odd_path = str(tmp_path / "capture.cu8"), str(tmp_path / "capture.raw"), str(tmp_path / "capture.bin")
    x.tofile(cu8_path)
    x.tofile(odd_path)
    convert(x, "cu8").tofile(i16_path)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode_file.py"), *a, "--call", "5000"],
                                    check=True, capture_output=True, text=True, timeout=300)
    want = run(i16_path, "--raw", "4", "--wideband", str(D), "--rate", str(R))
    got = run(cu8_path, "--wideband", str(D), "--rate", str(R), "--streams", "2")
    named = run(odd_path, "--wideband", str(D), "--rate", str(R), "--streams", "2", "--format", "cu8")
    assert want.stdout.count("!AIVDM") > 30
    assert got.stdout == want.stdout and named.stdout == want.stdout
