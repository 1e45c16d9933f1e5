"""Wideband in, on the device: every form of channeliser.hip -- each channeliser_kernel<K, NA> instance, the direct form
for each of its reasons, the carry copy, the run-time fall-back to the direct form for an output that is not aligned to
the fast form's vector store -- bit for bit against the NumPy restatement (tests/chan_ref.py) over the configuration
matrix of tests/chan_cases.py; rounding ties; the float64 bound on one shape; and run_wideband at K = 5 end to end."""
import ctypes as C

import numpy as np
import pytest

import chan_cases
import chan_ref
import iq_ref
from chan_cases import CASES, CASE_IDS
from gnuais_amd import synth

pytestmark = pytest.mark.gpu


def dev(x, device=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")


def configure(case, b):
    b.channeliser(case.D, case.R, list(case.offsets), taps=None if case.taps_kind == "default" else case.taps)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_form_bit_exact_ragged_and_reset(case):
    """Ragged calls (1-row calls shorter than T-1 read the old carry; 300-row calls span several segments), then
    reset() and the first two calls again (the carry and n are zero), every stream and offset against chan_ref."""
    from gnuais_amd import ReceiverBatch
    rng = np.random.default_rng(case.K * 7919 + case.D * 31 + case.T)
    chunks = case.chunks
    x = chan_cases.hard_wide(rng, sum(chunks), case.M)
    b = ReceiverBatch(case.M * case.K, max_len=max(case.rows))
    configure(case, b)
    ref = chan_ref.Channeliser(case.M, case.D, case.R, case.offsets, taps=case.taps)
    for rep, calls in enumerate((chunks, chunks[:2])):
        pos = 0
        for n in calls:
            got = b.channelise(dev(x[pos:pos + n])).cpu().numpy()
            want = ref.run(x[pos:pos + n])
            pos += n
            assert got.shape == (n // case.D, case.M * case.K, 2)
            assert np.array_equal(got, want), (case.name, rep, n, np.argwhere(got != want)[:5])
        b.reset()
        ref.reset()


def raw_channelise(b, xd, out_ptr):
    """gnuais_batch_channelise with a raw output address on torch's current stream; returns the status"""
    import torch
    s = torch.cuda.current_stream(xd.device)
    rc = b._lib.gnuais_batch_channelise(b._h, xd.data_ptr(), int(xd.shape[0]), C.c_void_p(out_ptr),
                                        C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc


@pytest.mark.parametrize("K,D,shifts", [(2, 3, (4, 8, 12, 0, 4)), (4, 2, (8, 16, 4, 12, 0))])
def test_unaligned_output_falls_back_to_the_direct_form(K, D, shifts):
    """The fast form stores K words per lane as one vector (8 bytes at K = 2, 16 at K = 4); an output address off that
    alignment takes the direct form at run time.  Calls alternate between the forms on one batch (the carry passes
    between them), every result equals chan_ref and nothing outside the output is written.  An output that is not
    4-byte aligned is refused and leaves the state alone."""
    import torch
    from gnuais_amd import ReceiverBatch, lib
    M = 65
    rows_per_call = (37, 1, 300, 2, 129)
    N = M * K
    rng = np.random.default_rng(K)
    x = chan_cases.hard_wide(rng, D * sum(rows_per_call), M)
    b = ReceiverBatch(N, max_len=max(rows_per_call))
    b.channeliser(D, 48000 * D, [-25000, 25000, 12345, -7][:K])     # default taps: the fast form, NA = 17
    assert chan_ref.fast_na(K, 16 * D + 1, D) == 17
    ref = chan_ref.Channeliser(M, D, 48000 * D, [-25000, 25000, 12345, -7][:K])
    fill = 0x5a5a
    pos = 0
    for rows, shift in zip(rows_per_call, shifts):
        n_words = rows * N
        buf = torch.full((2 * n_words + 64,), fill, dtype=torch.int16, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        xd = dev(x[pos:pos + rows * D])
        if rows == 1:                                   # refused: 2-byte aligned
            assert raw_channelise(b, xd, buf.data_ptr() + 2) == lib.E_ARG
            assert bool((buf == fill).all())
        assert raw_channelise(b, xd, buf.data_ptr() + shift) == lib.OK
        got = buf.cpu().numpy()
        e0, e1 = shift // 2, shift // 2 + 2 * n_words
        assert (got[:e0] == fill).all() and (got[e1:] == fill).all(), shift
        want = ref.run(x[pos:pos + rows * D])
        pos += rows * D
        assert np.array_equal(got[e0:e1].reshape(want.shape), want), (K, shift, rows)


def test_unaligned_input():
    """wide samples from a view 4, 8 or 12 bytes past a 16-byte boundary (the kernels read 4-byte words)"""
    import torch
    from gnuais_amd import ReceiverBatch
    case = {c.name: c for c in CASES}["k3_na17_bottom"]
    rng = np.random.default_rng(11)
    x = chan_cases.hard_wide(rng, sum(case.chunks), case.M)
    b = ReceiverBatch(case.M * case.K, max_len=max(case.rows))
    configure(case, b)
    ref = chan_ref.Channeliser(case.M, case.D, case.R, case.offsets, taps=case.taps)
    pos = 0
    for i, n in enumerate(case.chunks):
        e0 = 2 * (1 + i % 3)                            # int16 elements: 4, 8, 12 bytes
        buf = torch.zeros(2 * n * case.M + 8, dtype=torch.int16, device="cuda:0")
        view = buf[e0:e0 + 2 * n * case.M].view(n, case.M, 2)
        view.copy_(dev(x[pos:pos + n]))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        got = b.channelise(view).cpu().numpy()
        assert np.array_equal(got, ref.run(x[pos:pos + n])), (i, n)
        pos += n


@pytest.mark.parametrize("K,D,T", [(1, 1, 1), (2, 2, 2), (1, 1, 34), (5, 1, 1)])
def test_rounding_ties_in_the_filter_stage(K, D, T):
    """offset 0 and taps [16384, 0, ...]: acc / 32768 = mr / 2, a tie at every odd mixed value, of both signs; I, Q =
    +-16384 are ties of the mix.  Fast (K <= 2, T <= 33) and direct (T = 34, K = 5) forms; ties go towards +infinity."""
    from gnuais_amd import ReceiverBatch
    M = 65
    h = chan_cases.make_taps("tie", T, D, seed=0)
    rng = np.random.default_rng(T * 10 + K)
    x = rng.integers(-32768, 32768, (D * 400, M, 2)).astype(np.int16)
    m = rng.random((D * 400, M, 2)) < 0.3
    x[m] = rng.choice(np.array([16384, -16384, 1, -1, 3, -3, 32767, -32768], dtype=np.int16), int(m.sum()))
    b = ReceiverBatch(M * K, max_len=300)
    b.channeliser(D, 48000, [0] * K, taps=h)
    ref = chan_ref.Channeliser(M, D, 48000, [0] * K, taps=h)
    outs = []
    for lo, hi in ((0, D), (D, D * 100), (D * 100, D * 400)):
        got = b.channelise(dev(x[lo:hi])).cpu().numpy()
        assert np.array_equal(got, ref.run(x[lo:hi])), (K, D, T, lo)
        outs.append(got)
    # the tie rule itself: row m is ceil(mr / 2) of its sample mD + D-1
    mr, mi = chan_ref.Channeliser(M, D, 48000, [0], taps=h).mix(x[D - 1::D], 0)
    assert ((mr % 2 == 1) & (mr < 0)).any() and ((mr % 2 == 1) & (mr > 0)).any()
    out = np.concatenate(outs).reshape(-1, M, K, 2).astype(np.int64)
    for k in range(K):
        assert np.array_equal(out[:, :, k, 0], (mr[..., 0] + 1) // 2)
        assert np.array_equal(out[:, :, k, 1], (mi[..., 0] + 1) // 2)


def test_device_within_the_bound_of_float64_math():
    """chan_ref.ideal() in float64 against the device over ragged calls, asymmetric taps, D = 6, offsets of both
    signs: within chan_cases.ideal_bound(h) (derived in test_channeliser_cpu.test_restatement_within_the_bound_of_
    float64_math), mean error near zero"""
    from gnuais_amd import ReceiverBatch
    case = {c.name: c for c in CASES}["k3_na17_bottom"]
    h = case.taps
    x = chan_cases.unsaturated_wide(np.random.default_rng(5), sum(case.chunks), case.M, h)
    b = ReceiverBatch(case.M * case.K, max_len=max(case.rows))
    configure(case, b)
    parts, pos = [], 0
    for n in case.chunks:
        parts.append(b.channelise(dev(x[pos:pos + n])).cpu().numpy())
        pos += n
    err = chan_cases.ideal_errors(np.concatenate(parts), chan_ref.ideal(x, case.D, case.R, case.offsets, h))
    assert np.abs(err).max() <= chan_cases.ideal_bound(h), np.abs(err).max()
    assert abs(err.mean()) < 0.02 and np.abs(err).max() > 0.5, err.mean()


def frames_state(b):
    cnt = b.counters()
    return (b.drain_frames().tobytes(), cnt.tobytes(), b.pll_state().tobytes(), b.fsm_state().tobytes(),
            b.maxval().tobytes())


def test_run_wideband_at_k5_equals_run_iq_and_the_oracle():
    """K = 5 offsets: the direct form feeds the discriminator through the batch's I/Q scratch at N = 5M receivers.
    Frames, counters and PLL state against run_iq on the restated I/Q, frames against the CPU oracle."""
    from gnuais_amd import ReceiverBatch
    from oracle_lib import Oracle
    M, D = 8, 6
    offs = [-50000, -25000, 0, 25000, 50000]
    K, N = len(offs), len(offs) * M
    assert chan_ref.fast_na(K, 16 * D + 1, D) == 0
    n = 10 * synth.SLOT_BITS * 5 * D
    made = [synth.make_wideband_stream(n, D, 48000 * D, offs, seed=9, stream=s, sigma=300.0, occupancy=0.8)
            for s in range(M)]
    x = np.stack([m[0] for m in made], axis=1)
    chunks = [D * 1020, D, D * 3000, D * 333]
    chunks.append(n - sum(chunks))
    a = ReceiverBatch(N, max_len=max(chunks) // D)
    r = ReceiverBatch(N, max_len=max(chunks) // D)
    a.channeliser(D, 48000 * D, offs)
    ref = chan_ref.Channeliser(M, D, 48000 * D, offs)
    iq_all, pos = [], 0
    for c in chunks:
        iq = ref.run(x[pos:pos + c])
        iq_all.append(iq)
        a.run_wideband(dev(x[pos:pos + c]), sync=False)
        r.run_iq(dev(iq), sync=False)
        pos += c
    a.sync()
    r.sync()
    got, want = frames_state(a), frames_state(r)
    assert got == want
    o = Oracle(N)
    audio, _ = iq_ref.discriminate(np.concatenate(iq_all))
    o.run(audio)
    assert got[0] == o.frames().tobytes()
    cnt = a.counters()
    assert np.array_equal(np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1), o.counters())
    placed = sum(len(p) for m in made for p in m[1])
    assert cnt["receivedframes"].sum() >= 0.95 * placed and placed > 250
