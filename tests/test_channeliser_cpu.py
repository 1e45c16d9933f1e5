"""Wideband in, CPU side: the channeliser's definition (include/gnuais_hip.h) restated in NumPy (tests/chan_ref.py)
against the library's host tables, its intent (tuning, rejection, splitting, bounds), the argument checks, and the
CPU oracle behind the discriminator.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import chan_cases
import chan_ref
import iq_ref
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnuais_batch_channeliser", "gnuais_batch_run_wideband", "gnuais_batch_run_wideband_host",
               "gnuais_batch_channelise", "gnuais_channeliser_default_taps", "gnuais_channeliser_mixer_table",
               "gnuais_node_channeliser", "gnuais_node_run_wideband_host")


@pytest.fixture(scope="module")
def L():
    from gnuais_amd import lib
    return lib


def lib_taps(L, decim):
    h = L.load()
    n = C.c_int()
    assert h.gnuais_channeliser_default_taps(decim, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, dtype=np.int16)
    assert h.gnuais_channeliser_default_taps(decim, out.ctypes.data, out.size, C.byref(n)) == 0
    return out


def lib_mixer(L, rate, f):
    h = L.load()
    P = C.c_int()
    assert h.gnuais_channeliser_mixer_table(rate, f, None, 0, C.byref(P)) == 0
    out = np.zeros((P.value, 2), dtype=np.int16)
    assert h.gnuais_channeliser_mixer_table(rate, f, out.ctypes.data, P.value, C.byref(P)) == 0
    return out


@pytest.mark.parametrize("decim", [1, 2, 6, 8, 32, 64])
def test_default_taps_equal_the_formula(L, decim):
    got = lib_taps(L, decim)
    want = chan_ref.default_taps(decim)
    assert got.size == 16 * decim + 1
    assert np.array_equal(got, want)
    assert np.abs(want.astype(np.int64)).sum() <= 65535
    assert abs(int(want.astype(np.int64).sum()) - 32768) <= 16 * decim + 1


@pytest.mark.parametrize("rate,f", [(288000, 25000), (288000, -25000), (288000, 0), (48000, 1), (250000, -12345),
                                    (2048000, 25000), (96000, 96000), (1000, -3), (1 << 20, 1)])
def test_mixer_tables_equal_the_formula(L, rate, f):
    got = lib_mixer(L, rate, f)
    want = chan_ref.mixer_table(rate, f)
    assert got.shape == want.shape == (chan_ref.period(rate, f), 2)
    assert np.array_equal(got, want)


def test_default_design_response():
    """flat to 10 kHz, -6 dB near 18 kHz, stop band from 26 kHz at 48 kHz out"""
    for D in (2, 6, 8):
        h = chan_ref.default_taps(D).astype(np.float64)
        R = 48000 * D
        f = np.array([0, 10000, 18000, 26000, 50000], dtype=np.float64)
        H = np.abs(np.exp(-2j * np.pi * np.outer(f / R, np.arange(h.size))) @ h) / h.sum()
        db = 20 * np.log10(H)
        assert abs(db[1]) < 0.1 and -7.5 < db[2] < -5.0 and db[3] < -60 and db[4] < -60, (D, db)


def test_bad_arguments_are_refused(L):
    h = L.load()
    n = C.c_int()
    out = np.zeros(4, dtype=np.int16)
    assert h.gnuais_channeliser_default_taps(0, None, 0, C.byref(n)) == L.E_ARG
    assert h.gnuais_channeliser_default_taps(65, None, 0, C.byref(n)) == L.E_ARG
    assert h.gnuais_channeliser_default_taps(2, out.ctypes.data, 4, C.byref(n)) == L.E_ARG      # cap < 33
    assert h.gnuais_channeliser_mixer_table(0, 5, None, 0, C.byref(n)) == L.E_ARG
    assert h.gnuais_channeliser_mixer_table((1 << 20) + 1, 1, None, 0, C.byref(n)) == L.E_ARG  # period 2^20 + 1
    assert h.gnuais_channeliser_mixer_table(288000, 1, out.ctypes.data, 4, C.byref(n)) == L.E_ARG
    # the batch-level checks happen before any device is touched
    off = np.array([-25000, 25000], dtype=np.int32)
    for args in [(None, 6, 288000, off.ctypes.data, 2, None, 0)]:
        assert h.gnuais_batch_channeliser(*args) == L.E_ARG
    assert h.gnuais_batch_run_wideband(None, None, 6, None) == L.E_ARG
    assert h.gnuais_batch_run_wideband_host(None, None, 6) == L.E_ARG
    assert h.gnuais_batch_channelise(None, None, 6, None, None) == L.E_ARG
    assert h.gnuais_node_channeliser(None, 6, 288000, off.ctypes.data, 2, None, 0) == L.E_ARG
    assert h.gnuais_node_run_wideband_host(None, None, 6) == L.E_ARG


def tone(n, f, rate, amp=20000.0, phase=0.3):
    ph = phase + 2 * np.pi * f * np.arange(n) / rate
    return np.stack([np.rint(amp * np.cos(ph)), np.rint(amp * np.sin(ph))], axis=1).astype(np.int16)


def test_a_tone_lands_on_dc_of_its_offset_and_not_on_the_other():
    D, R = 6, 288000
    ch = chan_ref.Channeliser(1, D, R, [-25000, 25000])
    x = tone(60 * D * 40, 25000, R)[:, None, :]
    out = ch.run(x).astype(np.float64)            # [rows][2][2]
    settle = 40
    on = out[settle:, 1, 0] + 1j * out[settle:, 1, 1]
    off = out[settle:, 0, 0] + 1j * out[settle:, 0, 1]
    assert np.abs(on).min() > 0.99 * 20000 * 32767 / 32768 * 0.99
    assert np.ptp(on.real) <= 4 and np.ptp(on.imag) <= 4          # constant: DC
    assert 20 * np.log10(np.abs(off).max() / np.abs(on).mean()) < -60


@pytest.mark.parametrize("D,K", [(1, 1), (2, 3), (6, 2), (8, 2)])
def test_split_anywhere_equals_one_call(D, K):
    rng = np.random.default_rng(D * 10 + K)
    M = 3
    offs = [-25000, 25000, 12000][:K]
    x = rng.integers(-32768, 32768, (D * 90, M, 2)).astype(np.int16)
    x[::7] = -32768
    whole = chan_ref.Channeliser(M, D, 48000 * D, offs).run(x)
    for cuts in ([D], [D * 5, D * 6], [D * 89], [D * 30, D * 31, D * 60]):
        ch = chan_ref.Channeliser(M, D, 48000 * D, offs)
        parts, lo = [], 0
        for c in cuts + [x.shape[0]]:
            parts.append(ch.run(x[lo:c]))
            lo = c
        assert np.array_equal(np.concatenate(parts), whole), cuts


def test_worst_case_at_the_tap_bound_stays_in_int32():
    """sum |h| = 65535 with every mixed value at -32768 against the taps' signs: the largest |acc| the bounds allow"""
    T = 3
    h = np.array([32767, -32767, 1], dtype=np.int16)
    assert np.abs(h.astype(np.int64)).sum() == 65535
    # offset 0: C = 32767, S = 0 -> mr = sat16((32767 * I + 16384) >> 15); I = -32768 gives -32767
    ch = chan_ref.Channeliser(1, 1, 48000, [0], taps=h)
    x = np.zeros((8, 1, 2), dtype=np.int16)
    x[:, 0, 0] = [-32768, 32767, -32768, -32768, 32767, -32768, -32768, -32768]
    x[:, 0, 1] = -32768
    out = ch.run(x)
    mr = chan_ref.Channeliser(1, 1, 48000, [0], taps=np.array([32767], dtype=np.int16)).mix(x, 0)[0][:, 0, 0]
    acc = np.convolve(mr, h.astype(np.int64))[: x.shape[0]]
    assert np.abs(acc).max() + 16384 < 2 ** 31
    assert np.array_equal(out[:, 0, 0], np.clip((acc + 16384) >> 15, -32768, 32767))
    # the bound itself: 32768 * 65535 + 16384 < 2^31, and u, v at 2 * 32768 * 32767
    assert 32768 * 65535 + 16384 < 2 ** 31 and 2 * 32768 * 32767 < 2 ** 31
    # mixed values at their extremes through the full-scale mixer: u at -32768 * 32767 * 2 -> saturates to int16
    big = chan_ref.Channeliser(1, 1, 8, [1], taps=np.array([1], dtype=np.int16))
    mr, mi = big.mix(np.full((8, 1, 2), -32768, dtype=np.int16), 0)
    assert mr.min() >= -32768 and mr.max() <= 32767 and mi.min() >= -32768 and mi.max() <= 32767


def _decode(D=6, offs=(-25000, 25000), streams=2, slots=24, sigma=300.0):
    from oracle_lib import Oracle
    R = 48000 * D
    n = slots * synth.SLOT_BITS * 5 * D
    made = [synth.make_wideband_stream(n, D, R, offs, seed=5, stream=s, sigma=sigma, occupancy=0.7)
            for s in range(streams)]
    x = np.stack([m[0] for m in made], axis=1)
    iq = chan_ref.Channeliser(streams, D, R, offs).run(x)
    audio, _ = iq_ref.discriminate(iq)
    o = Oracle(streams * len(offs))
    o.run(audio)
    fr = o.frames()
    return made, fr


def test_oracle_decodes_both_offsets_and_neither_decodes_the_other():
    made, fr = _decode()
    K = 2
    placed = found = leak = 0
    for s, (_, per_off) in enumerate(made):
        for k in range(K):
            got = {bytes(f["payload"][: f["nbits"] // 8]) for f in fr if f["channel"] == s * K + k}
            mine = {p for _, p in per_off[k]}
            other = {p for _, p in per_off[1 - k]}
            placed += len(mine)
            found += len(mine & got)
            leak += len(other & got)
    assert placed > 40 and found == placed, (found, placed)
    assert leak == 0


def test_make_iq_stream_is_untouched_by_the_wideband_generator():
    a, pa = synth.make_iq_stream(6 * 1280, seed=7, channel=3)
    synth.make_wideband_stream(6 * 1280 * 2, 2, 96000, [-25000, 25000], seed=7, stream=3)
    b, pb = synth.make_iq_stream(6 * 1280, seed=7, channel=3)
    assert np.array_equal(a, b) and pa == pb


def test_channeliser_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name


def test_channeliser_build_is_checked_and_uses_dot2():
    mk = open(os.path.join(ROOT, "gnuais_amd", "csrc", "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/channeliser.s channeliser" in mk
    s_path = os.path.join(ROOT, "gnuais_amd", "csrc", "build", "channeliser.s")
    if os.path.exists(s_path):
        isa = open(s_path).read()
        assert "v_dot2c_i32_i16" in isa or "v_dot2_i32_i16" in isa


# ---- the configuration matrix (tests/chan_cases.py) and the references the device is held to ----

def test_the_matrix_picks_the_forms_it_names():
    """fast_na restates channeliser_fast_na(): buckets 4 / 8 / 17, 33 for K <= 2, else 0 = the direct form"""
    assert [chan_ref.fast_na(1, T, 1) for T in (1, 4, 5, 8, 9, 17, 18, 33, 34)] == [4, 4, 8, 8, 17, 17, 33, 33, 0]
    assert [chan_ref.fast_na(3, T, 1) for T in (17, 18)] == [17, 0]
    assert chan_ref.fast_na(5, 1, 1) == 0 and chan_ref.fast_na(0, 1, 1) == 0
    for c in chan_cases.CASES:
        assert chan_ref.fast_na(c.K, c.T, c.D) == c.na, c.name
        assert (c.na == 0) == bool(c.direct_reason), c.name
        assert c.taps.size == c.T and np.abs(c.taps.astype(np.int64)).sum() <= 65535, c.name
        assert all(chan_ref.period(c.R, f) <= 1 << 20 for f in c.offsets), c.name
    got = {(c.K, c.na) for c in chan_cases.CASES if c.na}
    assert got == {(K, na) for K in (1, 2, 3, 4) for na in (4, 8, 17, 33) if na != 33 or K <= 2}
    assert {c.direct_reason for c in chan_cases.CASES} == {"", "K>4", "ceil(T/D)>33", "ceil(T/D)>17,K>2"}
    assert {c.D for c in chan_cases.CASES} >= {1, 2, 3, 5, 7, 9, 16, 32, 63, 64}
    assert {c.M for c in chan_cases.CASES} >= {1, 63, 64, 65, 4096}
    assert max(c.T for c in chan_cases.CASES) == 1025
    top = {c.T // c.D for c in chan_cases.CASES if c.T % c.D == 0}                # T = b*D: ceil(T/D) = b
    bottom = {(c.T - 1) // c.D for c in chan_cases.CASES if (c.T - 1) % c.D == 0}   # T = b*D + 1: b + 1
    assert {4, 8, 17, 33} <= top and {4, 8, 17, 33} <= bottom, (top, bottom)


def test_the_matrix_reaches_every_instance_in_the_build():
    """Every int16 channeliser_kernel<K, NA, 0, false> the build holds is reached by a case of the matrix, and the int16
    direct and carry kernels are there, once in the whole build: a new bucket or instance fails here until the matrix
    tests it."""
    import re
    s_path = os.path.join(ROOT, "gnuais_amd", "csrc", "build", "channeliser.s")
    if not os.path.exists(s_path):
        pytest.skip("channeliser.s not built (make -C gnuais_amd/csrc)")
    isa = open(s_path).read()
    fast = re.findall(r"\.amdhsa_kernel \S*channeliser_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)EEEv", isa)
    assert {(f, r) for _, _, f, r in fast} == {("0", "0")}, "channeliser.s holds the int16 integer-ratio instances only"
    built = {(int(k), int(na)) for k, na, _, _ in fast}
    assert len(fast) == len(built) == 14, sorted(fast)
    assert built == {(c.K, c.na) for c in chan_cases.CASES if c.na}
    units = {n: open(os.path.join(os.path.dirname(s_path), n + ".s")).read() for n in ("channeliser_fmt", "resampler")}
    for form in ("direct", "carry"):
        sym = rf"\.amdhsa_kernel \S*channeliser_{form}_kernelILi0EEEv"
        assert len(re.findall(sym, isa)) == 1 and not any(re.findall(sym, u) for u in units.values()), form
    assert {c.direct_reason for c in chan_cases.CASES if not c.na} == {"K>4", "ceil(T/D)>33", "ceil(T/D)>17,K>2"}


@pytest.mark.parametrize("case", chan_cases.CASES, ids=chan_cases.CASE_IDS)
def test_restatement_within_the_bound_of_float64_math(case):
    """chan_ref over ragged calls against chan_ref.ideal() over the whole stream in float64 with no rounding.  Where
    nothing saturates, each component is within chan_cases.ideal_bound(h) = 1.5 sum |h| / 32768 + 0.5 of the ideal:
    the mixer table's C and S are each within 0.5 of 32767 cos, 32767 sin, so u = I C + Q S is within
    0.5 (|I| + |Q|) <= 32768 of 32767 (I cos + Q sin), 1.0 after the division by 32768; rounding the mix adds 0.5; the
    filter sums those errors weighted by |h[j]| / 32768 and rounds once more (0.5).  A wrong tap orientation, row
    phase (the last row ends on the call's last sample) or phase across calls is off by thousands.  The errors are
    rounding errors of both signs: their mean is near zero."""
    M = min(case.M, 2)
    h = case.taps
    x = chan_cases.unsaturated_wide(np.random.default_rng(case.T * 7 + case.D), sum(case.chunks), M, h)
    ch = chan_ref.Channeliser(M, case.D, case.R, case.offsets, taps=h)
    parts, pos = [], 0
    for n in case.chunks:
        parts.append(ch.run(x[pos:pos + n]))
        pos += n
    err = chan_cases.ideal_errors(np.concatenate(parts), chan_ref.ideal(x, case.D, case.R, case.offsets, h))
    bound = chan_cases.ideal_bound(h)
    assert np.abs(err).max() <= bound, (case.name, np.abs(err).max(), bound)
    assert abs(err.mean()) < 0.05, (case.name, err.mean())
    if err.size > 20000:
        assert np.abs(err).max() > 0.5                  # the check sees rounding at all


def test_ideal_bound_catches_a_reversed_filter_and_a_late_row():
    """the float64 check would fail if the restatement read its taps backwards or ended a row one sample late"""
    D, R, offs = 5, 240000, (-25000, 25000)
    h = chan_cases.make_taps("asym", 40, D, seed=1)
    x = chan_cases.unsaturated_wide(np.random.default_rng(2), D * 200, 2, h)
    y = chan_ref.ideal(x, D, R, offs, h)
    bound = chan_cases.ideal_bound(h)
    rev = chan_ref.Channeliser(2, D, R, offs, taps=h[::-1].copy()).run(x)
    assert np.abs(chan_cases.ideal_errors(rev, y)).max() > 10 * bound
    late = chan_ref.Channeliser(2, D, R, offs, taps=h).run(np.concatenate([np.zeros((1, 2, 2), np.int16), x[:-1]]))
    assert np.abs(chan_cases.ideal_errors(late, chan_ref.ideal(x, D, R, offs, h))).max() > 10 * bound


@pytest.mark.parametrize("name", ["k1_na4_T1", "k2_na4", "k3_na17_top", "k4_na8", "k5_direct", "k32_direct"])
def test_torch_reference_equals_the_restatement(name):
    """chan_ref.torch_channelise (the W3 test's reference on the device) against chan_ref on the CPU, one call from
    reset, with chunks smaller than M"""
    import torch
    c = {c.name: c for c in chan_cases.CASES}[name]
    M = min(c.M, 5)
    x = chan_cases.hard_wide(np.random.default_rng(c.T), c.D * 60, M)
    want = chan_ref.Channeliser(M, c.D, c.R, c.offsets, taps=c.taps).run(x)
    got = chan_ref.torch_channelise(torch.from_numpy(x), c.D, c.R, c.offsets, c.taps, chunk=2)
    assert got.dtype == torch.int16 and np.array_equal(got.numpy(), want)


def test_rounding_ties_go_up_in_both_stages():
    """(x + 16384) >> 15 rounds a tie towards +infinity: offset 0 (C = 32767, S = 0) makes I = 16384 a tie in the
    mix (16383.5 -> 16384) and I = -16384 one (-16383.5 -> -16383); taps [16384] make every odd mixed value a tie of
    the filter (mr / 2)"""
    ch = chan_ref.Channeliser(1, 1, 48000, [0], taps=np.array([16384], dtype=np.int16))
    I = np.array([16384, -16384, 3, -3, 1, -1, 32767, -32768, 5, -5], dtype=np.int16)
    x = np.stack([I, -I], axis=1)[:, None, :]
    mr, mi = ch.mix(x, 0)
    assert list(mr[:2, 0, 0]) == [16384, -16383]
    out = ch.run(x)[:, 0, :].astype(np.int64)
    assert np.array_equal(out[:, 0], (mr[:, 0, 0] + 1) // 2) and np.array_equal(out[:, 1], (mi[:, 0, 0] + 1) // 2)
    assert (mr[:, 0, 0] % 2 == 1).any() and ((mr[:, 0, 0] % 2 == 1) & (mr[:, 0, 0] < 0)).any()
