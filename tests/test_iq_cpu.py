"""Complex baseband in, CPU side: the discriminator's definition (include/gnuais_hip.h) restated in NumPy
(tests/iq_ref.py) against its intent, its edge cases, the carry, and the CPU oracle behind it; the new C ABI
symbols; the gfx950 ISA of iq_disc.hip.  No device."""
import os
import subprocess

import numpy as np
import pytest

import iq_ref
from gnuais_amd import params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = np.pi / 32768.0
NEW_SYMBOLS = ("gnuais_batch_run_iq", "gnuais_batch_run_iq_host", "gnuais_batch_discriminate",
               "gnuais_node_run_iq_host", "gnuais_node_run_iq")


def _wrap(d):
    """difference in output steps, on the circle of 65536 steps"""
    return (np.asarray(d, dtype=np.int64) + 32768) % 65536 - 32768


def test_constants_are_the_nearest_fp32_of_their_decimals():
    for k, d in iq_ref.DECIMALS.items():
        assert np.float32(float(d)).view(np.uint32) == np.float32(iq_ref.K[k]).view(np.uint32), k
    assert iq_ref.K["PI"] == np.float32(np.pi)
    assert iq_ref.K["HALF_PI"] == np.float32(np.pi / 2)
    assert iq_ref.K["G"] == np.float32(32768.0 / np.pi)


def test_restatement_within_two_steps_of_arctan2():
    rng = np.random.default_rng(11)
    n = 400000
    I, Q, Ip, Qp = (rng.integers(-32768, 32768, n) for _ in range(4))
    ext = np.array([-32768, -32767, -1, 0, 1, 32767])
    g = np.stack(np.meshgrid(ext, ext, ext, ext, indexing="ij"), axis=-1).reshape(-1, 4)
    I, Q, Ip, Qp = (np.concatenate([a, g[:, k]]) for k, a in enumerate((I, Q, Ip, Qp)))
    got = iq_ref.disc_pairs(I, Q, Ip, Qp).astype(np.int64)
    z = (I + 1j * Q) * np.conj(Ip + 1j * Qp)
    want = np.angle(z) / STEP
    nz = z != 0
    err = np.abs(_wrap(got[nz] - np.rint(want[nz]).astype(np.int64)))
    assert err.max() <= 2, err.max()
    assert np.all(got[~nz] == 0)


@pytest.mark.parametrize("omega", [0.0, 0.01, -0.05, 0.3142, 1.0, -2.0, 3.0])
def test_pure_rotation_gives_a_constant(omega):
    n = 2000
    ph = 0.7 + omega * np.arange(n)
    iq = np.stack([np.rint(20000 * np.cos(ph)), np.rint(20000 * np.sin(ph))], axis=1).astype(np.int16)
    out, _ = iq_ref.discriminate(iq[:, None, :])
    out = out[1:, 0].astype(np.int64)          # sample 0 follows the (0, 0) carry
    want = omega * 32768 / np.pi
    assert np.abs(out - want).max() <= 3, (out.min(), out.max(), want)


def test_ties_zeros_and_negative_zero():
    d = lambda I, Q, Ip, Qp: int(iq_ref.disc_pairs(I, Q, Ip, Qp))
    f = np.float32
    # |re| == |im|: t = 1, the polynomial at 1, no HALF_PI reflection (ay > ax is false)
    p1 = f(1) * (iq_ref.K["A1"] + f(1) * (iq_ref.K["A3"] + f(1) * (iq_ref.K["A5"] + f(1) * (iq_ref.K["A7"] + f(1) * iq_ref.K["A9"]))))
    q = int(np.rint(p1 * iq_ref.K["G"]))
    assert q in (8191, 8192)
    assert d(1, 1, 1, 0) == q            # re = 1, im = 1
    assert d(-1, 1, 1, 0) == int(np.rint((iq_ref.K["PI"] - p1) * iq_ref.K["G"]))   # re = -1, im = 1
    assert d(1, -1, 1, 0) == -q
    # zero pairs: mx == 0 -> 0
    assert d(0, 0, 0, 0) == 0
    assert d(5, -7, 0, 0) == 0
    assert d(0, 0, 123, 456) == 0
    # re = -0.0 (0 * -3 + -2 * 0): not < 0, so HALF_PI stays; a sign-bit test would give PI - HALF_PI (clipped 32767)
    assert d(0, -2, -3, 0) == int(np.rint(iq_ref.K["HALF_PI"] * iq_ref.K["G"])) == 16384
    # im = -0.0 (0 * -3 - 4 * 0) with re = -12: p = PI, not negated -> 32768 clipped to 32767 (a sign-bit test: -32768)
    assert d(4, 0, -3, 0) == 32767
    # exactly opposite, im = +0: +PI clips
    assert d(-5, 0, 5, 0) == 32767
    # just below -PI: the phase rounds to -PI in fp32, which does not clip
    assert d(-32768, -1, 32767, 0) == -32768


def test_split_anywhere_equals_one_call():
    rng = np.random.default_rng(5)
    iq = rng.integers(-32768, 32768, (300, 7, 2)).astype(np.int16)
    whole, carry_whole = iq_ref.discriminate(iq)
    for cut in (1, 2, 63, 64, 65, 150, 299):
        a, c = iq_ref.discriminate(iq[:cut])
        b, c2 = iq_ref.discriminate(iq[cut:], c)
        assert np.array_equal(np.concatenate([a, b]), whole), cut
        assert np.array_equal(c2, carry_whole)


def _decoded_share(sigma, sps=5, taps=None, pllinc=0, n_ch=6, slots=40, occupancy=0.8):
    from oracle_lib import Oracle
    total = slots * synth.SLOT_BITS * sps
    made = [synth.make_iq_stream(total, seed=21, channel=c, sps=sps, sigma=sigma, occupancy=occupancy)
            for c in range(n_ch)]
    iq = np.stack([m[0] for m in made], axis=1)
    audio, _ = iq_ref.discriminate(iq)
    o = Oracle(n_ch, taps=taps, pllinc=pllinc)
    o.run(audio)
    fr = o.frames()
    placed = found = 0
    for c, (_, pl) in enumerate(made):
        got = {bytes(f["payload"][: f["nbits"] // 8]) for f in fr if f["channel"] == c}
        placed += len(pl)
        found += sum(p in got for _, p in pl)
    return found, placed


def test_oracle_decodes_the_restated_audio_noiseless():
    found, placed = _decoded_share(0.0)
    assert placed > 150 and found == placed, (found, placed)


def test_oracle_decodes_the_restated_audio_at_default_noise():
    found, placed = _decoded_share(1500.0)
    assert placed > 150 and found >= 0.98 * placed, (found, placed)


def test_oracle_decodes_the_restated_audio_192k():
    found, placed = _decoded_share(0.0, sps=20, taps=params.taps_192k(), pllinc=params.PLLINC_192K, n_ch=3, slots=20)
    assert placed > 30 and found >= 0.95 * placed, (found, placed)


def test_make_stream_is_untouched_by_the_iq_generator():
    """make_iq_stream has its own random sequence: make_stream's output (bench input, golden files) is what it was."""
    a, pa = synth.make_stream(6 * 1280, seed=7, channel=3, occupancy=0.8)
    synth.make_iq_stream(6 * 1280, seed=7, channel=3)
    b, pb = synth.make_stream(6 * 1280, seed=7, channel=3, occupancy=0.8)
    assert np.array_equal(a, b) and pa == pb


def test_iq_symbols_declared_exported_and_bound():
    from gnuais_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name


def test_iq_disc_isa_has_the_correctly_rounded_division(tmp_path):
    src = os.path.join(ROOT, "gnuais_amd", "csrc", "iq_disc.hip")
    out = str(tmp_path / "iq_disc.s")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fPIC", "-Wno-unused-command-line-argument", "-S", "--cuda-device-only", src, "-o", out])
    isa = open(out).read()
    assert "iq_discriminator_kernel" in isa
    # one correctly rounded division per channel a lane owns, in each of the three lane widths (4 + 2 + 1)
    assert isa.count("v_div_fixup_f32") >= 7
    assert "v_rndne_f32" in isa
    mk = open(os.path.join(ROOT, "gnuais_amd", "csrc", "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/iq_disc.s iq_discriminator_kernel" in mk
