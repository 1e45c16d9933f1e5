"""The carrier-error stage (AFC), CPU side: the definition (include/gnuais_hip.h) restated in NumPy (tests/afc_ref.py)
against its intent -- cuts, tones, the edge cases -- and against the CPU oracle behind it on bursts with a carrier
error; the new C ABI symbols; the synthetic generators' new arguments; the gfx950 ISA of the discriminator's two
forms.  No device."""
import collections
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import afc_ref
import iq_ref
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnuais_batch_afc", "gnuais_batch_afc_estimate", "gnuais_batch_afc_apply", "gnuais_node_afc")


def test_phase_is_the_discriminators():
    """afc_ref.phase entered with the fp32 products of two pairs is iq_ref.disc_pairs"""
    rng = np.random.default_rng(3)
    I, Q, Ip, Qp = (rng.integers(-32768, 32768, 200000).astype(np.float32) for _ in range(4))
    re, im = (I * Ip) + (Q * Qp), (Q * Ip) - (I * Qp)
    assert np.array_equal(afc_ref.phase(re, im), iq_ref.disc_pairs(I, Q, Ip, Qp))


@pytest.mark.parametrize("W", [128, 1024])
def test_ragged_cuts_equal_one_call(W):
    rng = np.random.default_rng(W)
    cuts = [1, 63, 64, 65, 200, 1, 129, 1000, 7, 640]
    iq = rng.integers(-32768, 32768, (sum(cuts), 5, 2)).astype(np.int16)
    whole = afc_ref.Afc(5, W)
    want = whole.apply(iq)
    assert np.any(want[W // 2 + 1:] != 0) and not np.any(want[:W // 2])
    for c in (cuts, cuts[::-1], [len(iq) - 1, 1], [64] * (len(iq) // 64) + [len(iq) % 64]):
        c = [n for n in c if n]
        st = afc_ref.Afc(5, W)
        parts, pos = [], 0
        for n in c:
            parts.append(st.apply(iq[pos:pos + n]))
            pos += n
        assert np.array_equal(np.concatenate(parts), want), c
        assert np.array_equal(st.estimate(), whole.estimate())


@pytest.mark.parametrize("f", [-10000.0, -4000.0, -600.0, -37.0, 0.0, 300.0, 1500.0, 4000.0, 7777.0, 10000.0])
@pytest.mark.parametrize("W,rate", [(1024, 48000), (128, 48000), (4096, 192000)])
def test_noise_free_tone(f, W, rate):
    """After W rows every e_j is within 1 of round(f * 65536 / rate), and the corrected audio within 2 of 0: the
    polynomial's error is 0.1 unit, each of the two roundings (a and e) 0.5."""
    n = 3 * W + 777
    ph = 0.3 + 2.0 * np.pi * f / rate * np.arange(n)
    iq = np.stack([np.rint(30000 * np.cos(ph)), np.rint(30000 * np.sin(ph))], axis=1).astype(np.int16)[:, None, :]
    want = int(np.rint(f * 65536 / rate))
    st = afc_ref.Afc(1, W)
    es, out = [], []
    for lo in range(0, n, 64):                     # block by block: the estimate of every block is seen
        out.append(st.apply(iq[lo:lo + 64]))
        if lo + 64 > W:
            es.append(int(st.estimate()[0]))
    out = np.concatenate(out)[:, 0].astype(np.int64)
    assert len(es) > 2 * W // 64
    assert max(abs(e - want) for e in es) <= 1, (want, min(es), max(es))
    assert np.abs(out[W:]).max() <= 2, (out[W:].min(), out[W:].max())


def test_r_reaches_two_to_the_31():
    """all four values -32768: r = 2^31, which int32 does not hold.  A wrapped r (-2^31) would give a negative window
    sum and an estimate of +pi (32767) instead of 0."""
    iq = np.full((256, 1, 2), -32768, dtype=np.int16)
    r, i = afc_ref.products(iq[1:], iq[:-1])
    assert r.dtype == np.int64 and np.all(r == 2 ** 31) and np.all(i == 0)
    st = afc_ref.Afc(1, 128)
    out = st.apply(iq)
    # row 0 follows the (0, 0) carry: block 0 sums 63 products, the others 64
    assert st.blocks[:, 0, 0].tolist()[-2:] == [64 * 2 ** 31] * 2 and st.blocks.shape[0] <= 4
    assert np.all(out == 0) and st.estimate()[0] == 0
    # and with the sign turned in every second pair: r = -(2^31 - 32768) - ..., a true negative sum: +pi, clipped
    iq[1::2, 0, 0] = 32767
    iq[1::2, 0, 1] = 32767
    r, _ = afc_ref.products(iq[1:], iq[:-1])
    assert np.all(r == -2 * 32768 * 32767)
    st = afc_ref.Afc(1, 128)
    out = st.apply(iq)
    assert st.estimate()[0] == 32767
    # a[m] = 32767 (pi clips) minus e = 32767
    assert np.all(out[64 + 1:] == 0)


def test_zero_input_and_before_the_first_output_row():
    st = afc_ref.Afc(3, 256)
    assert np.all(st.estimate() == 0)
    out = st.apply(np.zeros((1000, 3, 2), dtype=np.int16))
    assert np.all(out == 0) and np.all(st.estimate() == 0)
    # rows before n = L are 0 whatever the input
    rng = np.random.default_rng(1)
    st = afc_ref.Afc(3, 256)
    out = st.apply(rng.integers(-32768, 32768, (128, 3, 2)).astype(np.int16))
    assert np.all(out == 0) and np.all(st.estimate() == 0)
    out = st.apply(rng.integers(-32768, 32768, (1, 3, 2)).astype(np.int16))      # n = 128 = L: m = 0, the first one
    assert np.any(st.estimate() != 0)


def test_window_sums_round_to_nearest_even_into_fp32():
    """int64 -> fp32 by hand: above 2^24 a float holds every second integer, above 2^45 every 2^22-th; a tie goes to the
    even mantissa"""
    f = np.float32
    cases = [(2 ** 24 + 1, 2.0 ** 24), (2 ** 24 + 3, 2.0 ** 24 + 4), (2 ** 24 + 2, 2.0 ** 24 + 2),
             (-(2 ** 24 + 1), -(2.0 ** 24)), (-(2 ** 24 + 3), -(2.0 ** 24 + 4)),
             (2 ** 45 + 2 ** 21, 2.0 ** 45), (2 ** 45 + 3 * 2 ** 21, 2.0 ** 45 + 2 ** 23),
             (2 ** 45 + 2 ** 21 + 1, 2.0 ** 45 + 2 ** 22), (2 ** 45 + 2 ** 21 - 1, 2.0 ** 45),
             (-(2 ** 45 + 2 ** 21 + 1), -(2.0 ** 45 + 2 ** 22)), (2 ** 46 - 1, 2.0 ** 46)]
    for v, want in cases:
        assert np.array(v, dtype=np.int64).astype(f) == f(want), v
    # and the estimate is the phase of the rounded sums: |re| and |im| that differ as integers tie as floats (t = 1,
    # no reflection), or keep their order
    p1 = f(1) * (iq_ref.K["A1"] + f(1) * (iq_ref.K["A3"] + f(1) * (iq_ref.K["A5"] + f(1) * (iq_ref.K["A7"] + f(1) * iq_ref.K["A9"]))))
    q = int(np.rint(p1 * iq_ref.K["G"]))
    assert int(afc_ref.estimate(2 ** 24 + 3, 2 ** 24 + 4)) == q
    assert int(afc_ref.estimate(-(2 ** 24 + 3), 2 ** 24 + 4)) == int(np.rint((iq_ref.K["PI"] - p1) * iq_ref.K["G"]))
    for (a, fa), (b, fb) in zip(cases[:-1], cases[1:]):
        assert afc_ref.estimate(a, b) == afc_ref.phase(f(fa), f(fb)), (a, b)
    assert int(afc_ref.estimate(0, 0)) == 0
    # a window of large equal products: SR = 16 * 64 * 2^30 + 1 ... the sums of a full-scale tone stay below 2^46
    assert 16384 * 2 ** 31 < 2 ** 46


# ---- decoding through iq_ref -> afc_ref -> the CPU oracle: gated bursts, sigma 1500, three seeds of 4 s ----
# Measured with this file's code (the blocked integer definition; frames decoded of 234 placed):
#   uncorrected (iq_ref -> oracle):  0 Hz 232   600 Hz 140   1500 Hz 0   4000 Hz 0
#   W =  512:  0 Hz 224   600 Hz 222   1500 Hz 215   4000 Hz 225
#   W = 1024:  0 Hz 225   600 Hz 228   1500 Hz 226   4000 Hz 224
#   W = 2048:  0 Hz 228   600 Hz 230   1500 Hz 225   4000 Hz 230
SEEDS = (1, 2, 3)
SLOTS = 150                                          # 4 s
MEASURED_W1024_AT_0HZ = 225
MEASURED_UNCORRECTED_AT_0HZ = 232

_counts = {}


def decoded(offset_hz, W):
    """(found, placed) over the three seeds; W = 0: the discriminator alone"""
    key = (offset_hz, W)
    if key in _counts:
        return _counts[key]
    from oracle_lib import Oracle
    found = placed = 0
    for seed in SEEDS:
        iq, pl = synth.make_iq_stream(SLOTS * synth.SLOT_BITS * 5, seed=seed, channel=0, sigma=1500.0, occupancy=0.5,
                                      gated=True, offset_hz=offset_hz)
        iq = iq[:, None, :]
        if W:                                        # the stage delays by W/2: push the end of the stream through
            audio = afc_ref.apply_stream(np.concatenate([iq, np.zeros((W // 2, 1, 2), dtype=np.int16)]), W)
        else:
            audio = iq_ref.discriminate(iq)[0]
        o = Oracle(1)
        o.run(audio)
        got = {bytes(f["payload"][: f["nbits"] // 8]) for f in o.frames()}
        placed += len(pl)
        found += sum(p in got for _, p in pl)
    _counts[key] = (found, placed)
    print(f"offset {offset_hz} Hz, W {W}: {found} of {placed}")
    return found, placed


def test_uncorrected_at_4_khz_decodes_nothing():
    found, placed = decoded(4000.0, 0)
    assert placed > 200 and found == 0, (found, placed)


@pytest.mark.parametrize("f", [600.0, 1500.0, 4000.0])
def test_corrected_count_does_not_depend_on_the_offset(f):
    """the estimator is shift-invariant up to rounding: within 2 % of the corrected count at 0 Hz"""
    c0, placed = decoded(0.0, 1024)
    cf, _ = decoded(f, 1024)
    assert placed > 200 and abs(cf - c0) <= 0.02 * c0, (f, cf, c0)


def test_corrected_at_0_hz_against_the_oracle_alone():
    """the price of the stage where there is nothing to correct: 225 of 234 against 232 uncorrected (3.0 %) at
    W = 1024; asserted: the measured count less 2 % (the spread between offsets), and a loss below 10 %"""
    c0, placed = decoded(0.0, 1024)
    u0, _ = decoded(0.0, 0)
    assert u0 >= 0.98 * MEASURED_UNCORRECTED_AT_0HZ, u0
    assert c0 >= 0.98 * MEASURED_W1024_AT_0HZ, (c0, u0, placed)
    assert c0 >= 0.90 * u0, (c0, u0)


def test_the_suggested_window_loses_no_more_than_its_neighbours():
    """2048 at 48 kHz (include/gnuais_hip.h): at 0 Hz 228, against 224 (512) and 225 (1024)"""
    c = {W: decoded(0.0, W)[0] for W in (512, 1024, 2048)}
    assert c[2048] >= c[1024] and c[2048] >= c[512], c


# ---- the generators' new arguments ----

def test_generator_defaults_are_what_they_were():
    n = 6 * 1280
    a, pa = synth.make_iq_stream(n, seed=7, channel=3)
    b, pb = synth.make_iq_stream(n, seed=7, channel=3, offset_hz=0.0, rate_hz=48000, gated=False)
    assert np.array_equal(a, b) and pa == pb
    w, _ = synth.make_wideband_stream(n * 2, 2, 96000, [-25000, 25000], seed=7, stream=1)
    v, _ = synth.make_wideband_stream(n * 2, 2, 96000, [-25000, 25000], seed=7, stream=1, offset_hz=0.0, gated=False)
    assert np.array_equal(w, v)
    # the same noise with and without the offset and the gate: no extra random numbers are drawn
    c, pc = synth.make_iq_stream(n, seed=7, channel=3, offset_hz=2500.0, gated=True)
    assert pc == pa and not np.array_equal(a, c)


def test_generator_offset_and_gate():
    n = 20 * 1280
    rate = 48000
    iq, pl = synth.make_iq_stream(n, seed=4, sigma=0.0, occupancy=0.6, offset_hz=3000.0, rate_hz=rate, gated=True)
    z = iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)
    on = np.abs(z) > 5000
    assert 0.3 < on.mean() < 0.8 and np.all(z[~on] == 0)            # off outside the bursts
    both = on[1:] & on[:-1]
    step = np.angle(z[1:] * np.conj(z[:-1]))[both]
    # over whole bursts the modulation averages out within its run-length imbalance: the mean step is the offset
    assert abs(step.mean() * rate / (2 * np.pi) - 3000.0) < 150.0
    # a burst lasts its bits plus 2 bits at either end
    first = pl[0][0] * 1280 + synth.START_OFFSET_BITS * 5
    assert on[first - 9] and not on[first - 11]


# ---- the boundary and the ISA ----

def test_afc_symbols_declared_exported_and_bound():
    from gnuais_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name
    assert '"afc_window"' in open(os.path.join(ROOT, "gnuais_amd", "csrc", "gnuais_capi.hip")).read()


def _kernel_histograms(isa):
    out, name = {}, None
    for line in isa.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = collections.Counter()
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        m = re.match(r"^\t([a-z][a-z0-9_]+)(\s|$)", line)
        if m and name:
            out[name][m.group(1)] += 1
    return out


# instructions, and a digest of the "mnemonic count" histogram, of iq_discriminator_kernel<4 / 2 / 1> as the commit before
# the AFC built them (the library's flags)
BEFORE_AFC = {4: (1140, "5711a6302ac4c425"), 2: (635, "e13b6526deca1cc5"), 1: (402, "ae91a6c85804d30d")}


def test_discriminator_isa_without_afc_is_unchanged_and_with_it_has_the_sums(tmp_path):
    csrc = os.path.join(ROOT, "gnuais_amd", "csrc")
    flags = "-O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-result -mllvm -pragma-unroll-threshold=200000"
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert f"--offload-arch=$(ARCH) {flags}" in mk.replace("\\\n         ", "")
    out = str(tmp_path / "iq_disc.s")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", *flags.split(),
                           "-Wno-unused-command-line-argument", "-S", "--cuda-device-only",
                           os.path.join(csrc, "iq_disc.hip"), "-o", out])
    hist = _kernel_histograms(open(out).read())
    for cpl, (total, digest) in BEFORE_AFC.items():
        off = [h for n, h in hist.items() if f"iq_discriminator_kernelILi{cpl}ELb0E" in n]
        on = [h for n, h in hist.items() if f"iq_discriminator_kernelILi{cpl}ELb1E" in n]
        assert len(off) == 1 and len(on) == 1, (cpl, list(hist))
        text = "\n".join(f"{m} {n}" for m, n in sorted(off[0].items()))
        assert sum(off[0].values()) == total, (cpl, sum(off[0].values()))
        assert hashlib.sha1(text.encode()).hexdigest()[:16] == digest, cpl
        # with the sums: the same divisions (one per sample), the packed dot product for r, 64-bit stores of the sums
        assert on[0]["v_div_fixup_f32"] == off[0]["v_div_fixup_f32"]
        assert on[0]["v_dot2c_i32_i16_e32"] + on[0]["v_dot2_i32_i16"] >= cpl
        assert sum(on[0].values()) > total
    assert "$(CHECK_RES) $(BUILD)/afc.s afc_estimate_kernel afc_apply_kernel" in mk
