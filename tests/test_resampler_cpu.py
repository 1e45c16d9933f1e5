"""Wideband in at a rational ratio, CPU side: the definition above gnuais_batch_resampler (include/gnuais_hip.h) restated in
NumPy (tests/resample_ref.py) against the library's host functions (default prototype, plan tables, time map), against
the integer channeliser's restatement at U = 1, against the float64 operation it approximates, its limits, and the CPU
oracle behind the discriminator.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chan_cases
import chan_ref
import frame_time_ref as ftr
import iq_ref
import resample_cases as cases
import resample_ref as rr
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
NEW_SYMBOLS = ("gnuais_batch_resampler", "gnuais_node_resampler", "gnuais_resampler_default_taps", "gnuais_resampler_plan",
               "gnuais_batch_time_map_ratio")
# the rates of the issue's table as ratios to 48 kHz
TABLE = [(24, 125), (6, 125), (3, 64), (2, 75), (3, 125), (3, 128), (12, 625), (3, 160), (2, 125), (3, 200), (1, 125), (3, 625)]


@pytest.fixture(scope="module")
def L():
    from gnuais_amd import lib
    return lib


def lib_taps(L, up, down):
    h = L.load()
    n = C.c_int()
    assert h.gnuais_resampler_default_taps(up, down, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, dtype=np.int16)
    assert h.gnuais_resampler_default_taps(up, down, out.ctypes.data, out.size, C.byref(n)) == 0
    return out


def lib_plan(L, up, down, taps=None):
    h = L.load()
    n_pairs, na, H = C.c_int(), C.c_int(), C.c_int()
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.int16)
    tp, tn = (None, 0) if t is None else (t.ctypes.data, t.size)
    assert h.gnuais_resampler_plan(up, down, tp, tn, None, 0, None, 0, C.byref(n_pairs), C.byref(na), C.byref(H)) == 0
    groups = np.zeros((up, 3), dtype=np.int32)
    pairs = np.zeros((n_pairs.value, na.value), dtype=np.uint32)
    assert h.gnuais_resampler_plan(up, down, tp, tn, groups.ctypes.data, groups.size, pairs.ctypes.data, pairs.size,
                                   C.byref(n_pairs), C.byref(na), C.byref(H)) == 0
    return groups, pairs, na.value, H.value


def test_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name


# ---- host functions ----

@pytest.mark.parametrize("up,down", cases.HOST_RATIOS)
def test_default_taps_equal_the_formula(L, up, down):
    got = lib_taps(L, up, down)
    want = rr.default_taps(up, down)
    assert got.size == 16 * down + 1
    assert np.array_equal(got, want)
    rr.check_config(up, down, want)


def test_default_design_sums_over_the_table_of_rates():
    """what the header says of the default design: the largest per-phase sum |h| is 48604 .. 48776 and the per-phase DC
    gain 32758 .. 32828 over the twelve rates, 32761 .. 32773 at 24/125; about 50500 at 5/6 and 2/3; all inside the
    int32 argument"""
    worst, gains = [], []
    for up, down in TABLE:
        h = rr.default_taps(up, down).astype(np.int64)
        worst.append(int(rr.phase_sums(up, h).max()))
        g = [int(h[phi::up].sum()) for phi in range(up)]
        gains += [min(g), max(g)]
        if (up, down) == (24, 125):
            assert (min(g), max(g)) == (32761, 32773)
    assert (min(worst), max(worst)) == (48604, 48776), worst
    assert (min(gains), max(gains)) == (32758, 32828), gains
    for up, down in ((5, 6), (2, 3)):
        assert 50400 < rr.phase_sums(up, rr.default_taps(up, down)).max() < 50600


@pytest.mark.parametrize("up,down", cases.HOST_RATIOS)
def test_plan_tables_equal_the_restatement(L, up, down):
    h = rr.default_taps(up, down)
    groups, pairs, na, H = lib_plan(L, up, down)
    w_groups, w_pairs, w_na, w_H = rr.plan(up, down, h)
    assert (na, H) == (w_na, w_H) == (17, -(-16 * down // up))
    assert np.array_equal(groups, w_groups)
    assert np.array_equal(pairs, w_pairs)
    first, size, base = groups[:, 0], groups[:, 1], groups[:, 2]
    assert size.sum() == down and set(size.tolist()) <= {down // up, -(-down // up)}
    assert first[0] == 0 and np.all(np.diff(first) > 0) and np.array_equal(first[1:], first[:-1] + size[:-1])
    assert np.array_equal(base, np.concatenate([[0], np.cumsum((size + 1) // 2)[:-1]]))
    # every tap of every phase exactly once: walk the table back to tap indices
    count = np.zeros(h.size, dtype=np.int64)
    for i in range(up):
        for q in range((size[i] + 1) // 2):
            for a in range(na):
                for half, k in enumerate((first[i] + 2 * q, first[i] + 2 * q + 1)):
                    v = (int(pairs[base[i] + q, a]) >> (16 * half)) & 0xffff
                    v -= 65536 if v >= 32768 else 0
                    j = (i + a) * down + down - 1 - k * up
                    if k < first[i] + size[i] and 0 <= j < h.size:
                        assert v == h[j]
                        count[j] += 1
                    else:
                        assert v == 0
    assert np.all(count == 1)


def test_plan_with_custom_taps_and_a_longer_prototype(L):
    rng = np.random.default_rng(3)
    for up, down, T in ((2, 3, 1), (3, 64, 17 * 64 + 1), (5, 6, 40), (3, 128, 16385)):
        h = cases.bounded_taps(rng, up, T)
        groups, pairs, na, H = lib_plan(L, up, down, h)
        w = rr.plan(up, down, h)
        assert na == w[2] == max(-(-T // down), 17) and H == w[3] == -(-(T - 1) // up)
        assert np.array_equal(groups, w[0]) and np.array_equal(pairs, w[1])


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """resample_plan.cpp is plain C++: built for the CPU with ASan + UBSan behind tests/c/resample_plan_main.cpp"""
    exe = str(tmp_path_factory.mktemp("plan") / "resample_plan.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "c", "resample_plan_main.cpp"),
                           os.path.join(CSRC, "resample_plan.cpp"), "-o", exe, "-lm"])
    return exe


SANITIZER_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_host_planning_under_the_sanitizers(plan_exe):
    args = [str(v) for r in cases.HOST_RATIOS + [(1, 1024), (64, 65), (63, 1024)] for v in r]
    p = subprocess.run([plan_exe] + args, capture_output=True, timeout=120, env=SANITIZER_ENV)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    assert "3/128 T 2049 NA 17 H 683 pairs 65" in lines and "2/3 T 49 NA 17 H 24 pairs 2" in lines, lines


@pytest.mark.parametrize("D", [1, 5, 6, 64])
def test_the_integer_pair_table_is_the_plan_at_up_1(plan_exe, D):
    """what gnuais_batch_channeliser puts on the device for its fast form: resample_plan() at U = 1 with
    channeliser_fast_na() accumulators is POLY[q][a] = (h[aD + D-1-2q], h[aD + D-2-2q]), zero where the tap index is
    >= T or the group's odd last sample has no partner.  T at both edges of every bucket: NA * D and NA * D - 1"""
    for K, NA in ((1, 4), (3, 8), (4, 17), (2, 33)):
        for T in (NA * D, NA * D - 1):
            p = subprocess.run([plan_exe, "poly", str(K), str(D), str(T)], capture_output=True, timeout=60, env=SANITIZER_ENV)
            assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
            lines = p.stdout.decode().strip().split("\n")
            assert lines[0].split() == [str(chan_ref.fast_na(K, T, D)), str((D + 1) // 2)], (K, D, T, lines[0])
            na = int(lines[0].split()[0])
            assert na == NA
            got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.uint32)
            h = ((np.arange(T) * 7919 + 13) % 4001 - 2000).astype(np.int16)

            def tap(j, r):
                return int(h[j]) & 0xffff if r < D and 0 <= j < T else 0

            want = np.array([[tap(a * D + D - 1 - 2 * q, 2 * q) | tap(a * D + D - 2 - 2 * q, 2 * q + 1) << 16
                              for a in range(na)] for q in range((D + 1) // 2)], dtype=np.uint32)
            assert got.shape == want.shape and np.array_equal(got, want), (K, D, T)


def test_bad_arguments_are_refused(L):
    h = L.load()
    n = C.c_int()
    out = np.zeros(8, dtype=np.int16)
    for up, down in ((0, 3), (65, 128), (3, 1025), (3, 3), (6, 5), (6, 128), (2, 4)):
        assert h.gnuais_resampler_default_taps(up, down, None, 0, C.byref(n)) == L.E_ARG, (up, down)
        assert h.gnuais_resampler_plan(up, down, None, 0, None, 0, None, 0, None, None, None) == L.E_ARG, (up, down)
    assert h.gnuais_resampler_default_taps(2, 3, out.ctypes.data, 8, C.byref(n)) == L.E_ARG          # cap < 49
    at = np.array([32767, 1, 32767, 32767, 1, 0], dtype=np.int16)          # U = 2: phases 65535 and 32768
    assert h.gnuais_resampler_plan(2, 3, at.ctypes.data, at.size, None, 0, None, 0, None, None, None) == 0
    over = at.copy()
    over[4] = 2                                                             # phase 0 at 65536
    assert h.gnuais_resampler_plan(2, 3, over.ctypes.data, over.size, None, 0, None, 0, None, None, None) == L.E_ARG
    assert "65535" in h.gnuais_last_error().decode()
    neg = np.array([-32768], dtype=np.int16)
    assert h.gnuais_resampler_plan(2, 3, neg.ctypes.data, 1, None, 0, None, 0, None, None, None) == L.E_ARG
    big = np.zeros(16386, dtype=np.int16)
    assert h.gnuais_resampler_plan(2, 3, big.ctypes.data, big.size, None, 0, None, 0, None, None, None) == L.E_ARG
    off = np.array([-25000, 25000], dtype=np.int32)
    assert h.gnuais_batch_resampler(None, 3, 128, 2048000, off.ctypes.data, 2, None, 0) == L.E_ARG
    assert h.gnuais_node_resampler(None, 3, 128, 2048000, off.ctypes.data, 2, None, 0) == L.E_ARG
    q = C.c_longlong()
    assert h.gnuais_batch_time_map_ratio(None, 2, C.byref(q), C.byref(q), C.byref(q)) == L.E_ARG


def test_the_restatement_refuses_what_the_definition_refuses():
    for up, down in ((6, 128), (3, 3), (6, 5), (3, 1025), (0, 5), (65, 128)):
        with pytest.raises(ValueError):
            rr.check_config(up, down)
    with pytest.raises(ValueError, match="phase sum"):
        rr.check_config(2, 3, [32767, 1, 32767, 32767, 2])
    rr.check_config(2, 3, [32767, 1, 32767, 32767, 1])
    with pytest.raises(ValueError, match="tap count"):
        rr.check_config(2, 3, np.zeros(16386))
    r = rr.Resampler(1, 3, 128, 2048000, [25000], max_len=30)
    with pytest.raises(ValueError, match="multiple"):
        r.run(np.zeros((127, 1, 2), dtype=np.int16))
    with pytest.raises(ValueError, match="max_len"):
        r.run(np.zeros((11 * 128, 1, 2), dtype=np.int16))                  # 33 rows
    assert r.run(np.zeros((10 * 128, 1, 2), dtype=np.int16)).shape == (30, 1, 2)


# ---- the restatement ----

@pytest.mark.parametrize("D", [1, 6, 64])
def test_up_1_equals_the_integer_channeliser_bit_for_bit(D):
    """the restatement's arithmetic at U = 1 is the integer channeliser's: default taps and custom ones, split calls
    (the entry refuses U = D = 1; the arithmetic is defined there all the same)"""
    rng = np.random.default_rng(D)
    M, offs = 2, [-25000, 25000, 12000]
    x = chan_cases.hard_wide(rng, D * 70, M)
    assert np.array_equal(rr.default_taps(1, D), chan_ref.default_taps(D))
    for taps in (None, cases.bounded_taps(rng, 1, 5 * D + 2)):
        a = chan_ref.Channeliser(M, D, 48000 * D, offs, taps=taps)
        b = rr.Resampler(M, 1, D, 48000 * D, offs, taps=taps, check=D > 1)
        assert b.H == b.T - 1
        for lo, hi in ((0, D), (D, 31 * D), (31 * D, 70 * D)):
            assert np.array_equal(a.run(x[lo:hi]), b.run(x[lo:hi])), (D, lo)


@pytest.mark.parametrize("up,down,K", [(2, 3, 3), (5, 6, 2), (3, 64, 2), (24, 125, 1)])
def test_split_anywhere_on_a_period_equals_one_call_and_reset_works(up, down, K):
    rng = np.random.default_rng(up * 1000 + down)
    M, P = 3, 40
    offs = cases.OFFS[K]
    x = chan_cases.hard_wide(rng, down * P, M)
    rate = 48000 * down // up
    whole = rr.Resampler(M, up, down, rate, offs).run(x)
    assert whole.shape == (P * up, M * K, 2)
    for cuts in ([1], [5, 6], [P - 1], [13, 14, 30]):
        r = rr.Resampler(M, up, down, rate, offs)
        parts, lo = [], 0
        for c in cuts + [P]:
            parts.append(r.run(x[lo * down:c * down]))
            lo = c
        assert np.array_equal(np.concatenate(parts), whole), cuts
        r.reset()
        assert np.array_equal(r.run(x), whole)


def test_worst_case_at_the_tap_bound_stays_in_int32():
    """every sample at -32768 on both components, prototypes whose phases sit at sum |h| = 65535: the largest |acc| the
    bounds allow, through the restatement's own assertion, and the bound itself"""
    assert 32768 * 65535 + 16384 < 2 ** 31
    for up, down in ((2, 3), (3, 64)):
        T = 16 * down
        h = np.zeros(T, dtype=np.int64)
        for phi in range(up):
            v = h[phi::up]
            v[:] = 0
            v[0], v[1], v[2] = 32767, 32767, 1
            h[phi::up] = v
        assert np.all(rr.phase_sums(up, h) == 65535)
        x = np.full((down * 20, 1, 2), -32768, dtype=np.int16)
        for f in (0, 25000):
            out = rr.Resampler(1, up, down, 48000 * down // up, [f], taps=h).run(x)
            assert out.min() == -32768 or out.max() == 32767        # saturated, not wrapped
        h[0] = -32767
        out = rr.Resampler(1, up, down, 48000 * down // up, [0], taps=h).run(x)
        assert out.shape[0] == 20 * up


# ---- filter quality ----

def quality_bound(up, taps):
    """chan_cases.ideal_bound() per phase: a row sums the mixed values' errors (<= 1.5 each) over the taps of one phase
    and rounds once more"""
    return 1.5 * float(rr.phase_sums(up, taps).max()) / 32768.0 + 0.5


@pytest.mark.parametrize("up,down", [(2, 3), (5, 6), (3, 64), (24, 125)])
def test_the_restatement_is_the_float_operation_within_the_rounding_bound(up, down):
    rng = np.random.default_rng(up + 7 * down)
    M, offs, rate = 2, [-25000, 25000], 48000 * down // up
    for h in (rr.default_taps(up, down), cases.bounded_taps(rng, up, 3 * down + 1)):
        x = chan_cases.unsaturated_wide(rng, down * 12, M, np.full(1, rr.phase_sums(up, h).max()))
        got = rr.Resampler(M, up, down, rate, offs, taps=h).run(x).astype(np.float64)
        got = (got[..., 0] + 1j * got[..., 1]).reshape(-1, M, 2)
        bound = quality_bound(up, h)

        def err(y):
            return max(np.abs(got.real - y.real).max(), np.abs(got.imag - y.imag).max())

        e = err(rr.ideal(x, up, down, rate, offs, h))
        print(f"{up}/{down} T {h.size}: error {e:.3f}, bound {bound:.3f}")
        assert e <= bound, (up, down, h.size, e, bound)
        if h.size != 16 * down + 1:
            # the bound tells a wrong tap order and a wrong phase from the right ones (the default design is symmetric,
            # so the reversal is tested on the asymmetric prototype)
            assert err(rr.ideal(x, up, down, rate, offs, h[::-1])) > 10 * bound
        assert err(rr.ideal(x, up, down, rate, offs, h, tick_shift=1)) > 10 * bound


@pytest.mark.parametrize("up,down", [(3, 128), (24, 125)])
def test_default_design_response(up, down):
    """the figures of the integer channeliser's response test at the 48 kHz output: flat to 10 kHz, -6 dB near 18 kHz,
    stop band from 26 kHz; the prototype runs at up * in rate = 48000 * down"""
    h = rr.default_taps(up, down).astype(np.float64)
    R = 48000.0 * down
    f = np.array([0, 10000, 18000, 26000, 50000], dtype=np.float64)
    H = np.abs(np.exp(-2j * np.pi * np.outer(f / R, np.arange(h.size))) @ h) / h.sum()
    db = 20 * np.log10(H)
    assert abs(db[1]) < 0.1 and -7.5 < db[2] < -5.0 and db[3] < -66 and db[4] < -66, (up, down, db)


@pytest.mark.parametrize("up,down", [(3, 128), (24, 125)])
def test_a_tone_lands_on_dc_of_its_offset_and_not_on_the_other(up, down):
    rate = 48000 * down // up
    n = down * 80
    ph = 0.3 + 2 * np.pi * 25000 * np.arange(n) / rate
    x = np.stack([np.rint(20000 * np.cos(ph)), np.rint(20000 * np.sin(ph))], axis=1).astype(np.int16)[:, None, :]
    out = rr.Resampler(1, up, down, rate, [-25000, 25000]).run(x).astype(np.float64)
    settle = 40
    on = out[settle:, 1, 0] + 1j * out[settle:, 1, 1]
    off = out[settle:, 0, 0] + 1j * out[settle:, 0, 1]
    assert np.abs(on).min() > 0.98 * 20000
    # constant up to the phases' DC gains, which differ by rounding (32758 .. 32828 of 32768: 20000 * 70 / 32768 = 43)
    assert np.ptp(on.real) <= 48 and np.ptp(on.imag) <= 48
    assert 20 * np.log10(np.abs(off).max() / np.abs(on).mean()) < -60


# ---- decode ----

def capture(up, down, streams=1, slots=24, seed=5, sigma=300.0, occupancy=0.7, **kw):
    n = slots * synth.SLOT_BITS * 5 * down // up
    assert n % down == 0
    made = [synth.make_resampled_wideband_stream(n, up, down, (-25000, 25000), seed=seed, stream=s, sigma=sigma,
                                                 occupancy=occupancy, **kw) for s in range(streams)]
    return np.stack([m[0] for m in made], axis=1), made


@pytest.mark.parametrize("up,down", [(3, 128), (24, 125)])
def test_oracle_decodes_both_offsets_and_neither_decodes_the_other(up, down):
    from oracle_lib import Oracle
    x, made = capture(up, down)
    iq = rr.Resampler(1, up, down, 48000 * down // up, [-25000, 25000]).run(x)
    audio, _ = iq_ref.discriminate(iq)
    o = Oracle(2)
    o.run(audio)
    fr = o.frames()
    placed = found = leak = 0
    for k in range(2):
        got = {bytes(f["payload"][: f["nbits"] // 8]) for f in fr if f["channel"] == k}
        mine = {p for _, p in made[0][1][k]}
        other = {p for _, p in made[0][1][1 - k]}
        placed += len(mine)
        found += len(mine & got)
        leak += len(other & got)
    print(f"{up}/{down}: {found} of {placed} placed frames decoded, {leak} leaked")
    assert placed == 35 and found == placed, (found, placed)
    assert leak == 0


def test_existing_generators_are_untouched_by_the_new_one():
    a, pa = synth.make_wideband_stream(6 * 1280 * 2, 2, 96000, [-25000, 25000], seed=7, stream=3)
    synth.make_resampled_wideband_stream(1280 * 3, 2, 3, [-25000, 25000], seed=7, stream=3)
    b, pb = synth.make_wideband_stream(6 * 1280 * 2, 2, 96000, [-25000, 25000], seed=7, stream=3)
    assert np.array_equal(a, b) and pa == pb
    # up = 1 keeps every sample: the integer generator's signal, then the same noise
    c, pc = synth.make_resampled_wideband_stream(6 * 1280 * 2, 1, 2, [-25000, 25000], seed=7, stream=3, sigma=0.0)
    d, pd = synth.make_wideband_stream(6 * 1280 * 2, 2, 96000, [-25000, 25000], seed=7, stream=3, sigma=0.0)
    assert np.array_equal(c, d) and pc == pd


# ---- time map ----

def test_time_map_ratio_arithmetic():
    assert rr.time_map_ratio(1, 6, 97) == (6, 1) + ftr.time_map("wideband", decim=6, chan_taps=97)[1:]
    assert rr.time_map_ratio(3, 128, 2049) == (128, 3, -18 * 128 + 127 - 1024)
    assert rr.time_map_ratio(3, 128, 2049, afc_window=1024) == (128, 3, (-18 - 512) * 128 + 127 - 1024)
    # the tagged formatter needs no sibling: floor(floor(a / den) / rate) == floor(a / (den * rate)), negatives included
    for a in (-10 ** 7, -4097, -1, 0, 5, 4096 * 3 - 1, 10 ** 9 + 7):
        for den, rate in ((3, 2048000), (24, 250000), (1, 48000)):
            assert (a // den) // rate == a // (den * rate)


@pytest.mark.parametrize("W", [0, 1024])
def test_slot_of_every_decoded_frame_at_3_128(W):
    """the slot test of the frame times at a rational ratio, with no tolerance: the input index of every decoded frame,
    (t * num + off) // den, lies in the slot its payload was placed in, floor(index * U / (1280 * D))"""
    import afc_ref
    up, down, M = 3, 128, 1
    x, made = capture(up, down, streams=M, seed=3, sigma=500.0, occupancy=0.8, gated=True, offset_hz=2500.0 if W else 0.0)
    placed = [p for m in made for p in m[1]]                # receiver s*K + k
    r = rr.Resampler(M, up, down, 2048000, [-25000, 25000])
    periods = x.shape[0] // down
    cuts = [0, 1, 400, 401, 3000, 3002, 7000, periods]
    num, den, off = rr.time_map_ratio(up, down, 2049, afc_window=W)
    ref = ftr.FrameTimeRef(2 * M)
    afc, carry, checked = (afc_ref.Afc(2 * M, W) if W else None), None, 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        iq = r.run(x[a * down:b * down])
        if afc:
            audio = afc.apply(iq)
        else:
            audio, carry = iq_ref.discriminate(iq, carry)
        ref.run(audio)
        fr, times = ref.drain()
        for f, t in zip(fr, times):
            assert t >= 0
            index = (int(t) * num + off) // den
            slot = (index * up) // (1280 * down)
            want = dict(placed[int(f["channel"])]).get(slot)
            assert want is not None and bytes(f["payload"][: int(f["nbits"]) // 8]) == want, (int(f["channel"]), int(t), slot)
            checked += 1
    decoded = int(ref.o.counters()[:, 0].sum())
    assert checked >= decoded and decoded > 20, (checked, decoded)


# ---- build ----

def test_resampler_build_is_checked_and_holds_exactly_the_instances_the_matrix_reaches():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/resampler.s channeliser" in mk
    objs = mk.split("OBJS :=")[1].split("\n\n")[0]
    assert "$(BUILD)/resampler.o" in objs and "$(BUILD)/resample_plan.o" in objs
    s_path = os.path.join(CSRC, "build", "resampler.s")
    assert os.path.exists(s_path), "resampler.s not built (make -C gnuais_amd/csrc)"
    isa = open(s_path).read()
    found = re.findall(r"\.amdhsa_kernel \S*channeliser_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)EEEv", isa)
    assert {r for _, _, _, r in found} == {"1"}, "resampler.s holds the rational instances only"
    built = {(int(k), int(na), int(f)) for k, na, f, _ in found}
    fast, direct = cases.instances_reached()
    assert built == fast, (sorted(built - fast), sorted(fast - built))
    assert len(found) == len(built) == 16
    # the direct form and the carry copy are the integer ratio's: each format's exists exactly once in the whole build
    units = [isa] + [open(os.path.join(CSRC, "build", name)).read() for name in ("channeliser.s", "channeliser_fmt.s")]
    for form in ("direct", "carry"):
        sym = rf"\.amdhsa_kernel \S*channeliser_{form}_kernelILi(\d+)EEEv"
        assert sorted(int(f) for u in units for f in re.findall(sym, u)) == [0, 1, 2, 3], form
        assert not re.findall(sym, isa), form
    assert direct == {0, 1, 2, 3}
    assert "v_dot2c_i32_i16" in isa
    # a translation unit of its own: the integer ratio's objects hold no rational instance
    for u in units[1:]:
        assert not re.findall(r"channeliser_kernelILi\d+ELi\d+ELi\d+ELb1E", u)
