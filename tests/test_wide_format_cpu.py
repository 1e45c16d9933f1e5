"""Sample formats of wideband input, CPU side: gnuais_convert_samples (the host's use of the formulas the kernels share,
gnuais_amd/csrc/wide_format.h) against the NumPy restatement (tests/wide_format_ref.py) and the closed forms of the
definition; the same unit built by itself under ASan + UBSan; the new symbols and their argument checks; the build's
instances against the matrix of tests/wide_format_cases.py; the capture-file readers; and decoding of captures quantised
to each format through the restated chain.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chan_cases
import chan_ref
import iq_ref
import wide_format_cases as cases
from wide_format_ref import DTYPE, FORMATS, PAIR_BYTES, VALUE, convert, quantise
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
NEW_SYMBOLS = ("gnuais_batch_run_wideband_fmt", "gnuais_batch_run_wideband_fmt_host", "gnuais_batch_channelise_fmt",
               "gnuais_node_run_wideband_fmt_host", "gnuais_sample_format_bytes", "gnuais_convert_samples")


@pytest.fixture(scope="module")
def L():
    from gnuais_amd import lib
    return lib


def lib_convert(L, x, fmt):
    """gnuais_convert_samples on an array of components [..][2] -> int16 of the same shape"""
    x = np.ascontiguousarray(x)
    assert x.dtype == DTYPE[fmt] and x.shape[-1] == 2
    out = np.full(x.shape, 0x5a5a, dtype=np.int16)
    assert L.load().gnuais_convert_samples(VALUE[fmt], x.ctypes.data, x.size // 2, out.ctypes.data) == L.OK
    return out


def all_byte_pairs(fmt):
    """all 65 536 (I, Q) pairs of an 8-bit format"""
    b = np.arange(256, dtype=np.uint8).view(DTYPE[fmt])
    return np.stack(np.meshgrid(b, b, indexing="ij"), axis=-1).reshape(-1, 2)


def cf32_vectors():
    """the special values, ties and clamp points in both components against each other, then 10^6 random values over
    +-1.2"""
    s = cases.cf32_specials()
    grid = np.stack(np.meshgrid(s, s, indexing="ij"), axis=-1).reshape(-1, 2)
    rnd = np.random.default_rng(12).uniform(-1.2, 1.2, (500000, 2)).astype(np.float32)
    return np.concatenate([grid, rnd])


@pytest.mark.parametrize("fmt", ["cu8", "cs8"])
def test_every_8_bit_pair_equals_the_restatement_and_the_closed_form(L, fmt):
    x = all_byte_pairs(fmt)
    assert x.shape == (65536, 2)
    got = lib_convert(L, x, fmt)
    assert np.array_equal(got, convert(x, fmt))
    v = x.astype(np.int64)
    if fmt == "cu8":
        assert np.array_equal(got, 256 * v - 32640) and np.array_equal(got, (2 * v - 255) * 128)
        word = ((v << 8) ^ 0x8080) & 0xffff                       # on the 16-bit word
        assert np.array_equal(got.astype(np.int64) & 0xffff, word)
        assert got.min() == -32640 and got.max() == 32640
    else:
        assert np.array_equal(got, 256 * v)
        assert got.min() == -32768 and got.max() == 32512


def test_cu8_is_the_customary_float_conversion_at_full_scale_32640(L):
    """(u - 127.5) / 127.5 at a full scale of 32640 is (u - 127.5) * 256: exact in float64, and equal to v for all 256"""
    u = np.arange(256, dtype=np.uint8)
    v = lib_convert(L, np.stack([u, u[::-1]], axis=1), "cu8")
    want = (u.astype(np.float64) - 127.5) * 256.0
    assert np.array_equal(want, (u.astype(np.float64) - 127.5) / 127.5 * 32640.0)
    assert np.array_equal(v[:, 0].astype(np.float64), want) and np.array_equal(v[::-1, 1].astype(np.float64), want)


def test_cf32_special_values_ties_and_clamp_points(L):
    s = cases.cf32_specials()
    got = lib_convert(L, np.stack([s, s[::-1]], axis=1), "cf32")
    want = cases.cf32_expected(s)
    assert np.array_equal(got[:, 0], want) and np.array_equal(got[::-1, 1], want)
    assert np.array_equal(convert(s, "cf32"), want)
    named = {0.0: 0, -0.0: 0, 1.0: 32767, -1.0: -32768, np.inf: 32767, -np.inf: -32768, 1e30: 32767, -1e30: -32768}
    for x, v in named.items():
        assert lib_convert(L, np.array([[x, x]], dtype=np.float32), "cf32").tolist() == [[v, v]], x
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))                  # 32767.998 -> 32768 -> clamped
    assert lib_convert(L, np.array([[below_one, -below_one]], dtype=np.float32), "cf32").tolist() == [[32767, -32768]]
    nan = np.array([0x7fc00000, 0xffc00000], dtype=np.uint32).view(np.float32)
    assert lib_convert(L, nan[None, :], "cf32").tolist() == [[0, 0]]
    sub = np.array([0x007fffff, 0x80000001], dtype=np.uint32).view(np.float32)
    assert lib_convert(L, sub[None, :], "cf32").tolist() == [[0, 0]]
    for k in range(-6, 7):                                                      # ties go to the even neighbour
        t = np.float32((k + 0.5) / 32768.0)
        assert float(t) * 32768.0 == k + 0.5
        even = k if k % 2 == 0 else k + 1
        assert lib_convert(L, np.array([[t, t]], dtype=np.float32), "cf32").tolist() == [[even, even]], k
    hi = cases.neighbours(32767.5 / 32768.0)                                    # 32767.498, 32767.5, 32767.502
    lo = cases.neighbours(-32768.5 / 32768.0)
    assert float(hi[1]) * 32768.0 == 32767.5 and float(lo[1]) * 32768.0 == -32768.5
    assert lib_convert(L, np.stack([hi, lo], axis=1), "cf32").tolist() == [[32767, -32768]] * 3
    just_inside = np.float32(32767.25 / 32768.0)
    assert lib_convert(L, np.array([[just_inside, -just_inside]], dtype=np.float32), "cf32").tolist() == [[32767, -32767]]


def test_cf32_random_values_and_cs16(L):
    x = cf32_vectors()
    assert x.size >= 10 ** 6
    got = lib_convert(L, x, "cf32")
    assert np.array_equal(got, convert(x, "cf32"))
    sample = np.random.default_rng(3).choice(x.shape[0], 20000, replace=False)
    assert np.array_equal(got[sample].ravel(), cases.cf32_expected(x[sample].ravel()))
    y = chan_cases.hard_wide(np.random.default_rng(4), 5000, 3)
    assert np.array_equal(lib_convert(L, y, "cs16"), y) and np.array_equal(convert(y, "cs16"), y)


def test_quantise_is_the_nearest_code_of_each_format():
    """the test inputs of the decode checks: convert(quantise(v)) is within half a step of v (128 for the 8-bit formats,
    0 for cf32 and cs16) except where the format's range ends"""
    v = np.arange(-32768, 32768, dtype=np.int16)
    for fmt, half in (("cs16", 0), ("cf32", 0), ("cu8", 128), ("cs8", 128)):
        back = convert(quantise(v, fmt), fmt).astype(np.int64)
        inside = (v >= -32640) & (v <= 32512)
        assert np.abs(back - v)[inside].max() <= half, fmt


SAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "gnuais_hip.h"
/* argv: fmt in out; `in` holds the pairs; they are converted from a buffer one byte off any alignment */
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int fmt = atoi(argv[1]);
    const int pair = gnuais_sample_format_bytes(fmt);
    if (pair <= 0) return 3;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 4;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *buf = malloc((size_t) bytes + 1);
    if (fread(buf + 1, 1, (size_t) bytes, f) != (size_t) bytes) return 5;
    fclose(f);
    const size_t n = (size_t) bytes / (size_t) pair;
    int16_t *out = malloc(sizeof(int16_t) * 2 * n + 2);
    if (gnuais_convert_samples(fmt, buf + 1, n, out) != GNUAIS_OK) return 6;
    if (gnuais_convert_samples(4, buf, n, out) != GNUAIS_E_ARG || gnuais_convert_samples(-1, buf, n, out) != GNUAIS_E_ARG) return 7;
    if (gnuais_convert_samples(fmt, NULL, n, out) != GNUAIS_E_ARG || gnuais_convert_samples(fmt, buf, n, NULL) != GNUAIS_E_ARG) return 8;
    if (gnuais_sample_format_bytes(4) != GNUAIS_E_ARG || gnuais_sample_format_bytes(-1) != GNUAIS_E_ARG) return 9;
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, sizeof(int16_t), 2 * n, f) != 2 * n) return 10;
    fclose(f);
    free(out);
    free(buf);
    return 0;
}
'''


def test_convert_samples_standalone_under_asan_and_ubsan(tmp_path):
    """wide_format.cpp has no HIP dependency: g++ builds it by itself with -fsanitize=address,undefined (and
    -ffp-contract=off, as the library does), and the same vectors give the restatement's values, from an input that is
    not aligned to anything"""
    exe = str(tmp_path / "convert.bin")
    main_c = tmp_path / "main.c"
    main_c.write_text(SAN_MAIN)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", *san, "-I", inc, "-c", str(main_c), "-o",
                           str(tmp_path / "main.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *san, "-c",
                           os.path.join(CSRC, "wide_format.cpp"), "-o", str(tmp_path / "wide_format.o")])
    subprocess.check_call(["g++", *san, str(tmp_path / "main.o"), str(tmp_path / "wide_format.o"), "-o", exe])
    vectors = {"cu8": all_byte_pairs("cu8"), "cs8": all_byte_pairs("cs8"), "cf32": cf32_vectors(),
               "cs16": chan_cases.hard_wide(np.random.default_rng(4), 5000, 3).reshape(-1, 2)}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for fmt, x in vectors.items():
        src, dst = str(tmp_path / f"{fmt}.in"), str(tmp_path / f"{fmt}.out")
        np.ascontiguousarray(x).tofile(src)
        r = subprocess.run([exe, str(VALUE[fmt]), src, dst], capture_output=True, env=env, timeout=300)
        assert r.returncode == 0, (fmt, r.returncode, r.stderr.decode()[-2000:])
        got = np.fromfile(dst, dtype=np.int16).reshape(-1, 2)
        assert np.array_equal(got, convert(x, fmt)), fmt


def test_format_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name
    for fmt in FORMATS:
        assert re.search(rf"#define GNUAIS_FMT_{fmt.upper()}\s+{VALUE[fmt]}\b", hdr), fmt
        assert L.FORMATS[fmt] == (VALUE[fmt], DTYPE[fmt])
        assert handle.gnuais_sample_format_bytes(VALUE[fmt]) == PAIR_BYTES[fmt]
    assert (L.FMT_CS16, L.FMT_CU8, L.FMT_CS8, L.FMT_CF32) == (0, 1, 2, 3)


def test_bad_format_arguments_are_refused_without_a_device(L):
    h = L.load()
    x = np.zeros(8, dtype=np.uint8)
    out = np.zeros(8, dtype=np.int16)
    for bad in (4, -1, 1 << 20):
        assert h.gnuais_sample_format_bytes(bad) == L.E_ARG
        assert h.gnuais_convert_samples(bad, x.ctypes.data, 1, out.ctypes.data) == L.E_ARG
    assert h.gnuais_convert_samples(1, None, 1, out.ctypes.data) == L.E_ARG
    assert h.gnuais_convert_samples(1, x.ctypes.data, 1, None) == L.E_ARG
    assert h.gnuais_convert_samples(1, x.ctypes.data, 0, out.ctypes.data) == L.OK         # nothing to do
    for fmt in (0, 1, 2, 3, 4):
        assert h.gnuais_batch_run_wideband_fmt(None, fmt, x.ctypes.data, 6, None) == L.E_ARG
        assert h.gnuais_batch_run_wideband_fmt_host(None, fmt, x.ctypes.data, 6) == L.E_ARG
        assert h.gnuais_batch_channelise_fmt(None, fmt, x.ctypes.data, 6, out.ctypes.data, None) == L.E_ARG
        assert h.gnuais_node_run_wideband_fmt_host(None, fmt, x.ctypes.data, 6) == L.E_ARG


def test_the_format_kernels_are_built_checked_and_reached_by_the_matrix():
    """channeliser_fmt.s holds exactly the cs16 set of (K, NA) instances for each of cu8, cs8 and cf32 (42 fast-form
    kernels), a direct and a carry kernel per format -- each exactly once in the whole build -- and v_dot2c_i32_i16; its
    Makefile line runs the resource check; and tests/wide_format_cases.py reaches every one of them, as the cs16 rule
    of test_channeliser_cpu.py asks"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/channeliser_fmt.s channeliser" in mk
    assert "$(BUILD)/channeliser_fmt.o" in mk.split("OBJS :=")[1].split("\n\n")[0]
    assert "$(BUILD)/wide_format.o" in mk.split("OBJS :=")[1].split("\n\n")[0]
    s_path = os.path.join(CSRC, "build", "channeliser_fmt.s")
    assert os.path.exists(s_path), "channeliser_fmt.s not built (make -C gnuais_amd/csrc)"
    isa = open(s_path).read()
    fast = re.findall(r"\.amdhsa_kernel \S*channeliser_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)EEEv", isa)
    assert {r for _, _, _, r in fast} == {"0"}, "channeliser_fmt.s holds integer-ratio instances only"
    built = {(int(k), int(na), int(f)) for k, na, f, _ in fast}
    cs16 = {(c.K, c.na) for c in chan_cases.CASES if c.na}
    assert len(cs16) == 14 and len(fast) == len(built) == 42, sorted(built)
    assert built == {(K, na, VALUE[fmt]) for K, na in cs16 for fmt in cases.FORMATS}
    assert built == {(c.K, c.na, VALUE[fmt]) for fmt, c in cases.CASES if c.na}
    want_f = {VALUE[fmt] for fmt in cases.FORMATS}
    others = [open(os.path.join(CSRC, "build", n)).read() for n in ("channeliser.s", "resampler.s")]
    for form in ("direct", "carry"):
        sym = rf"\.amdhsa_kernel \S*channeliser_{form}_kernelILi(\d+)EEEv"
        here = [int(f) for f in re.findall(sym, isa)]
        assert sorted(here) == sorted(want_f), (form, here)                   # each format's, once
        assert not any(int(f) in want_f for o in others for f in re.findall(sym, o)), form
    for fmt in cases.FORMATS:
        assert {c.direct_reason for f, c in cases.CASES if f == fmt and not c.na} == \
            {"K>4", "ceil(T/D)>33", "ceil(T/D)>17,K>2"}, fmt
    assert "v_dot2c_i32_i16" in isa
    assert "v_perm_b32" in isa and "v_rndne_f32" in isa          # the byte placement and the fp32 rounding
    cs16_unit = open(os.path.join(CSRC, "build", "channeliser.s")).read()
    assert not re.findall(r"channeliser\w*_kernelILi\d+ELi\d+ELi[123]E", cs16_unit) and \
        not re.findall(r"channeliser_(?:direct|carry)_kernelILi[123]E", cs16_unit)   # none of these formats' kernels there


def test_the_kernels_and_the_host_share_the_header_of_the_formulas():
    """the kernels and gnuais_convert_samples both take the conversions from wide_format.h"""
    for name in ("wide_kernels.h", "wide_format.cpp"):
        assert '#include "wide_format.h"' in open(os.path.join(CSRC, name)).read(), name


def test_read_iq_raw_and_format_of_path(tmp_path):
    from gnuais_amd import io
    ext = {".cu8": "cu8", ".cs8": "cs8", ".cs16": "cs16", ".cf32": "cf32", ".u8": "cu8", ".s8": "cs8", ".s16": "cs16",
           ".f32": "cf32", ".cfile": "cf32"}
    for e, fmt in ext.items():
        assert io.format_of_path(f"/somewhere/capture{e}") == fmt
        assert io.format_of_path(f"capture.2024{e.upper()}") == fmt
    for bad in ("capture.wav", "capture", "capture.cu8.gz"):
        with pytest.raises(ValueError):
            io.format_of_path(bad)
    rng = np.random.default_rng(8)
    for fmt in FORMATS:
        for M in (1, 3):
            x = cases.hard_input(rng, 50, M, fmt) if fmt != "cs16" else chan_cases.hard_wide(rng, 50, M)
            path = str(tmp_path / f"x{M}.{fmt}")
            with open(path, "wb") as f:
                f.write(x.tobytes() + x.tobytes()[: PAIR_BYTES[fmt] * M - 1])       # a partial trailing row
            got = io.read_iq_raw(path, fmt, M)
            assert got.dtype == DTYPE[fmt] and got.shape == (50, M, 2)
            assert got.tobytes() == x.tobytes()
    with pytest.raises(ValueError):
        io.read_iq_raw(path, "cs32")


def weak_capture(streams=4, slots=40):
    """the issue's capture: a weak signal (amplitude 1500, sigma 225: 32 codes of a u8) at D = 6, both AIS offsets"""
    D, R, offs = 6, 288000, [-25000, 25000]
    n = slots * synth.SLOT_BITS * 5 * D
    made = [synth.make_wideband_stream(n, D, R, offs, seed=9, stream=s, amplitude=1500.0, sigma=225.0, occupancy=0.8)
            for s in range(streams)]
    return np.stack([m[0] for m in made], axis=1), [m[1] for m in made], D, R, offs


@pytest.mark.parametrize("fmt", FORMATS)
def test_quantised_captures_decode_through_the_restated_chain(fmt):
    """convert -> chan_ref -> iq_ref -> the CPU oracle on a capture quantised to each format: at least 0.95 of the
    frames placed are decoded (the K = 5 wideband test's bar; 255 placed, 255 decoded for every format when this was
    written)"""
    from oracle_lib import Oracle
    x, placed, D, R, offs = weak_capture()
    q = quantise(x, fmt)
    if fmt == "cu8":
        assert 100 <= q.min() and q.max() <= 155                 # five bits of the eight
    iq = chan_ref.Channeliser(x.shape[1], D, R, offs).run(convert(q, fmt))
    audio, _ = iq_ref.discriminate(iq)
    o = Oracle(x.shape[1] * len(offs))
    o.run(audio)
    got = {(int(f["channel"]), bytes(f["payload"][: f["nbits"] // 8])) for f in o.frames()}
    want = {(s * len(offs) + k, p) for s, per_off in enumerate(placed) for k in range(len(offs)) for _, p in per_off[k]}
    assert len(want) > 200
    assert len(want & got) >= 0.95 * len(want), (fmt, len(want & got), len(want))
