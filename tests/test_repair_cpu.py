"""Single-symbol repair, CPU side: gnuais_repair_candidate -- the host's use of the trial text the kernel runs
(gnuais_amd/csrc/hdlc_repair.h) -- against the brute-force restatement (tests/repair_ref.py) in count, position, nbits
and payload; the restatement's deframer against the oracle's counters; what the repair buys on noisy streams; the
ambiguous fixtures; the same unit built by itself under ASan + UBSan; the new symbols and their argument checks.
No device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hip_cpu_build
import repair_ref as rr
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
NEW_SYMBOLS = ("gnuais_batch_repair", "gnuais_batch_repaired", "gnuais_repair_candidate", "gnuais_node_repair",
               "gnuais_node_repaired")
SEEDS = (10, 11, 12, 13, 14, 15)
SIGMAS = (5000, 6000)


@pytest.fixture(scope="module")
def L():
    from gnuais_amd import lib
    return lib


def host_repair(L, raw):
    """gnuais_repair_candidate -> (count, p, n', payload bytes) shaped like repair_ref.repair()"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    pl = np.full(53, 0xA5, dtype=np.uint8)
    n, p = C.c_int(-7), C.c_int(-7)
    k = L.load().gnuais_repair_candidate(raw.ctypes.data, int(raw.size), pl.ctypes.data, C.byref(n), C.byref(p))
    if k != 1:
        assert (n.value, p.value) == (-7, -7) and np.all(pl == 0xA5), "outputs written without a unique trial"
        return (k, None, None, None)
    assert not pl[n.value // 8:].any(), "payload not zero behind nbits / 8 bytes"
    return (1, p.value, n.value, pl[: n.value // 8].tobytes())


def ref_repairs(raws):
    """repair_ref.repair() of many records, those of one length side by side"""
    raws = [np.asarray(r, dtype=np.uint8) for r in raws]
    out = [None] * len(raws)
    by_len = {}
    for i, r in enumerate(raws):
        by_len.setdefault(r.size, []).append(i)
    for n, idx in by_len.items():
        for k in range(0, len(idx), 32):
            part = idx[k:k + 32]
            for i, passing in zip(part, rr.brute_force_many([raws[j] for j in part])):
                out[i] = (1,) + passing[0] if len(passing) == 1 else (len(passing), None, None, None)
    return out


def assert_host_equals_ref(L, raws, what):
    want = ref_repairs(raws)
    for i, (r, w) in enumerate(zip(raws, want)):
        assert host_repair(L, r) == w, (what, i, len(r))
    return want


def flipped(raw, p):
    out = np.array(raw, dtype=np.uint8)
    out[p] ^= 1
    out[p + 1] ^= 1
    return out


@pytest.fixture(scope="module")
def streams():
    """per (sigma, seed): the placed payloads, the restatement's deframer and the oracle's counters"""
    from oracle_lib import Oracle
    out = {}
    for sigma in SIGMAS:
        for seed in SEEDS:
            x, placed = synth.make_stream(4 * 48000, seed=seed, amplitude=12000.0, sigma=float(sigma), occupancy=0.5)
            o = Oracle(1)
            bits = o.run(x[:, None], want_bits=True)["bits"][0]
            d = rr.Deframer()
            d.feed(bits)
            out[sigma, seed] = (placed, d, o.counters()[0], o.frames())
    return out


def test_the_restated_deframer_counts_what_the_oracle_counts(streams):
    for key, (placed, d, counters, frames) in streams.items():
        assert (d.received, d.lost, d.lost2) == tuple(int(v) for v in counters), key
        good = [f for f in d.closed if f["good"]]
        assert [f["end_bit"] & 0xFFFFFFFF for f in good] == [int(e) for e in frames["end_bit"]], key
        assert [f["payload"] for f in good] == [bytes(f["payload"][: f["nbits"] // 8]) for f in frames], key


def test_failed_candidates_of_noisy_streams_host_equals_restatement_and_repairs_are_placed_frames(L, streams):
    """every CRC-failed candidate of make_stream, seeds 10-15 at sigma 5000 and 6000; each repaired payload is one the
    generator placed; the counts are printed (DESIGN.md 4.13 holds them)"""
    for sigma in SIGMAS:
        n_placed = n_good = n_failed = n_repaired = n_several = 0
        for seed in SEEDS:
            placed, d, _, _ = streams[sigma, seed]
            payloads = {p for _, p in placed}
            failed = [f for f in d.closed if not f["good"]]
            got = assert_host_equals_ref(L, [f["raw"] for f in failed], ("stream", sigma, seed))
            for k, p, n, payload in got:
                n_several += k > 1
                if k == 1:
                    assert payload in payloads, (sigma, seed, p, n)
                    n_repaired += 1
            n_placed += len(placed)
            n_good += d.received
            n_failed += len(failed)
        print(f"sigma {sigma}: placed {n_placed}, decoded {n_good}, CRC-failed candidates {n_failed}, "
              f"repaired {n_repaired} (each a placed payload), more than one trial passes {n_several}")
        assert n_repaired >= 1


@pytest.mark.parametrize("nbytes,count", [(21, 8), (53, 2)])
def test_valid_frames_with_one_pair_inverted_at_every_position(L, nbytes, count):
    """168- and 424-bit frames: a pair inverted at every p is repaired to the frame, at p, unless another trial passes
    too (then host and restatement agree on the count)"""
    rng = np.random.default_rng(100 + nbytes)
    total = 0
    for _ in range(count):
        payload = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        raw = rr.candidate_raw(payload)
        recs = [flipped(raw, p) for p in range(raw.size - 1)]
        got = assert_host_equals_ref(L, recs, ("every p", nbytes))
        for p, g in enumerate(got):
            assert g[0] >= 1, p                                    # the trial that undoes the error always passes
            if g[0] == 1:
                assert g[1:] == (p, 8 * nbytes, payload), p
        total += len(recs)
    print(f"{nbytes * 8}-bit frames: {total} records")


def stuffed_with_map(payload):
    """candidate_raw(payload) and, for each bit of payload + FCS, its index among the raw bits"""
    fcs = synth.crc16_x25(payload)
    body = np.unpackbits(np.frombuffer(payload + bytes([fcs & 0xFF, fcs >> 8]), dtype=np.uint8), bitorder="little")
    raw, where, ones = [], [], 0
    for b in body:
        where.append(len(raw))
        raw.append(int(b))
        ones = ones + 1 if b else 0
        if ones == 5:
            raw.append(0)
            ones = 0
    raw += [0, 1, 1, 1, 1, 1]
    raw = np.array(raw, dtype=np.uint8)
    assert np.array_equal(raw, rr.candidate_raw(payload))
    return raw, where


@pytest.mark.parametrize("nbytes", [21, 53])
def test_pairs_that_change_the_stuffing_and_pairs_at_the_edges(L, nbytes):
    rng = np.random.default_rng(7 + nbytes)
    payload = bytearray(rng.integers(0, 256, nbytes, dtype=np.uint8))
    payload[5:8] = bytes([0x00, 0x1F, 0x00])        # 0 11111 (0) 000: a stuffed zero in the frame
    payload[10:13] = bytes([0x00, 0x2F, 0x00])      # 0 1111 0 1 00
    payload = bytes(payload)
    raw, where = stuffed_with_map(payload)
    a = where[6 * 8 + 4]                            # the fifth 1 of 0x1f; raw[a + 1] is the stuffed zero
    assert raw[a - 4:a + 3].tolist() == [1, 1, 1, 1, 1, 0, 0]
    b = where[11 * 8 + 4]                           # the 0 of 1111 0 1
    assert raw[b - 4:b + 2].tolist() == [1, 1, 1, 1, 0, 1]
    last = raw.size - 2
    cases = {
        "the error destroyed a stuffed zero, the trial makes one": flipped(raw, a),
        "the error made a stuffed zero, the trial destroys one": flipped(raw, b),
        "six 1s as received": flipped(raw, a + 1),
        "p = 0": flipped(raw, 0),
        "p = rawlen - 2": flipped(raw, last),
        "p = rawlen - 6 (the closing flag's 0)": flipped(raw, raw.size - 6),
        "p = 30": flipped(raw, 30), "p = 31": flipped(raw, 31), "p = 32": flipped(raw, 32),
        "p = 62": flipped(raw, 62), "p = 63": flipped(raw, 63), "p = 64": flipped(raw, 64),
        "untouched": raw,
    }
    got = assert_host_equals_ref(L, list(cases.values()), "edges")
    by_name = dict(zip(cases, got))
    assert by_name["the error destroyed a stuffed zero, the trial makes one"] == (1, a, 8 * nbytes, payload)
    assert by_name["the error made a stuffed zero, the trial destroys one"] == (1, b, 8 * nbytes, payload)
    assert by_name["six 1s as received"] == (1, a + 1, 8 * nbytes, payload)
    for name, p in (("p = 0", 0), ("p = rawlen - 2", last), ("p = 30", 30), ("p = 31", 31), ("p = 32", 32)):
        g = by_name[name]
        assert g[0] >= 1 and (g[0] > 1 or g[1:] == (p, 8 * nbytes, payload)), name
    assert by_name["untouched"][0] == 0             # no pair keeps a valid frame valid: (1 + x) x^k is no multiple


def test_records_at_the_limit_of_a_candidate_and_garbage(L):
    payload = b"\xff" * 53                          # 424 bits, a stuffed zero behind every five: the longest record
    raw = rr.candidate_raw(payload)
    assert 520 <= raw.size <= 537
    ps = sorted(set(range(0, raw.size - 1, 9)) | {raw.size - 2, raw.size - 3, raw.size - 7})
    got = assert_host_equals_ref(L, [flipped(raw, p) for p in ps], "limit")
    assert sum(g[0] == 1 and g[3] == payload for g in got) >= len(ps) // 2
    # 449 stored bits and more: nothing is well formed
    long_raw = np.concatenate([np.tile(np.array([1, 0], dtype=np.uint8), 230), [0, 1, 1, 1, 1, 1]])
    assert host_repair(L, long_raw)[0] == 0 and rr.repair(long_raw)[0] == 0
    rng = np.random.default_rng(5)
    junk = []
    for n in (2, 3, 5, 6, 7, 23, 31, 32, 33, 64, 65, 200, 576):
        for _ in range(6):
            r = rng.integers(0, 2, n, dtype=np.uint8)
            r[-6:] = [0, 1, 1, 1, 1, 1][-min(n, 6):]
            junk.append(r)
    assert_host_equals_ref(L, junk, "junk")
    # four random raw bits inverted in valid frames: what passes is the same in both
    recs = []
    for _ in range(60):
        raw = rr.candidate_raw(bytes(rng.integers(0, 256, 21, dtype=np.uint8)))
        r = raw.copy()
        r[rng.choice(raw.size, 4, replace=False)] ^= 1
        recs.append(r)
    assert_host_equals_ref(L, recs, "four bits")
    assert host_repair(L, np.zeros(577, dtype=np.uint8))[0] == 0        # more than a candidate record holds
    assert host_repair(L, np.zeros(1, dtype=np.uint8))[0] == 0 and host_repair(L, np.zeros(0, dtype=np.uint8))[0] == 0


def ambiguous_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "repair_ambiguous.json")) as f:
        return json.load(f)


def test_candidates_that_two_trials_repair_stay_lost(L):
    fixtures = ambiguous_fixtures()
    assert len(fixtures) >= 4
    for fx in fixtures:
        raw = flipped(rr.candidate_raw(bytes.fromhex(fx["payload"])), fx["p1"])
        passing = rr.brute_force(raw)
        assert [t[0] for t in passing] == fx["passes_at"] and len(passing) == 2 and fx["p1"] in fx["passes_at"], fx
        assert passing[0][2] != passing[1][2]                      # two different frames, both with a good CRC
        assert host_repair(L, raw) == (2, None, None, None), fx


SAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "gnuais_hip.h"
/* argv: in out; in: records of (int32 n_raw, n_raw bytes); out: per record int32 count, p, nbits + 53 payload bytes */
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t n;
    while (fread(&n, sizeof n, 1, f) == 1) {
        uint8_t *raw = malloc((size_t) n + 1);        /* exactly n bytes are the record's: one more keeps n = 0 legal */
        if (n && fread(raw, 1, (size_t) n, f) != (size_t) n) return 4;
        uint8_t *payload = malloc(53);
        for (int i = 0; i < 53; ++i) payload[i] = 0xA5;
        int nbits = -7, pos = -7;
        uint8_t *exact = malloc((size_t) n ? (size_t) n : 1);
        for (int i = 0; i < n; ++i) exact[i] = raw[i];
        const int32_t k = gnuais_repair_candidate(exact, n, payload, &nbits, &pos);
        const int32_t head[3] = {k, pos, nbits};
        if (fwrite(head, sizeof head, 1, g) != 1 || fwrite(payload, 1, 53, g) != 53) return 5;
        free(exact);
        free(payload);
        free(raw);
    }
    uint8_t none[53];
    int a = 0, b = 0;
    if (gnuais_repair_candidate(NULL, 5, none, &a, &b) != GNUAIS_E_ARG) return 6;
    fclose(f);
    fclose(g);
    return 0;
}
'''


def test_repair_candidate_standalone_under_asan_and_ubsan(L, tmp_path):
    """hdlc_repair.cpp has no HIP dependency: g++ builds it by itself with -fsanitize=address,undefined, and the records
    of the edge cases, the limit, junk of every length and the ambiguous fixtures give what the library gives"""
    exe = str(tmp_path / "repair.bin")
    main_c = tmp_path / "main.c"
    main_c.write_text(SAN_MAIN)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-c",
                           str(main_c), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-c", os.path.join(CSRC, "hdlc_repair.cpp"),
                           "-o", str(tmp_path / "hdlc_repair.o")])
    subprocess.check_call(["g++", *san, str(tmp_path / "main.o"), str(tmp_path / "hdlc_repair.o"), "-o", exe])
    rng = np.random.default_rng(9)
    recs = []
    for nbytes in (21, 53):
        raw = rr.candidate_raw(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)))
        recs += [flipped(raw, p) for p in range(raw.size - 1)]
    full = rr.candidate_raw(b"\xff" * 53)
    recs += [flipped(full, p) for p in (0, 31, full.size - 2)]
    recs += [flipped(rr.candidate_raw(bytes.fromhex(fx["payload"])), fx["p1"]) for fx in ambiguous_fixtures()]
    for n in (0, 1, 2, 5, 31, 32, 33, 575, 576, 577, 1000):
        recs.append(rng.integers(0, 2, n, dtype=np.uint8))
        recs.append(np.ones(n, dtype=np.uint8))
    src, dst = str(tmp_path / "records.in"), str(tmp_path / "records.out")
    with open(src, "wb") as f:
        for r in recs:
            f.write(np.int32(r.size).tobytes() + r.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = np.fromfile(dst, dtype=np.dtype([("head", "<i4", (3,)), ("payload", "u1", (53,))]))
    assert out.size == len(recs)
    for rec, o in zip(recs, out):
        k, p, n, payload = host_repair(L, rec)
        if k == 1:
            assert o["head"].tolist() == [1, p, n] and o["payload"][: n // 8].tobytes() == payload
        else:
            assert o["head"].tolist() == [k, -7, -7] and np.all(o["payload"] == 0xA5)


def test_the_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path):
    """hdlc_repair.hip compiled for the CPU behind tests/c/hip_cpu (a thread per lane, a block at a time) under ASan +
    UBSan and run through launch_hdlc_repair(): over the candidate ring of 40 noisy channels -- good, failed and abandoned records, ring slots that
    wrap, junk behind rawlen, stamps above 2^32, several passes per block -- the records it appends and its counters are
    the restatement's.  The kernel's control flow cannot be checked on a device by the CPU suite; this is that check."""
    from oracle_lib import FRAME_DTYPE, Oracle
    exe = hip_cpu_build.build("repair_kernel_main.cpp", tmp_path / "repair_kernel.bin")
    N, K, rows = 40, 64, 36000
    x = np.stack([synth.make_stream(rows, seed=20, channel=c, amplitude=12000.0, sigma=6000.0, occupancy=0.5)[0]
                  for c in range(N)], axis=1)
    bits = Oracle(N).run(x, want_bits=True)["bits"]
    cand = np.zeros((N, K, 20), dtype=np.uint32)
    first, count = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
    rng = np.random.default_rng(3)
    want, want_rep = [], np.zeros(N, dtype=np.int32)
    for c in range(N):
        d = rr.Deframer()
        d.feed(bits[c])
        first[c] = rng.integers(0, 200)
        j = 0
        for f in d.closed:
            raw = f["raw"]
            nw = (raw.size + 31) // 32
            rec = cand[c, (first[c] + j) % K]
            e = f["end_bit"] + (c % 3) * (1 << 32)
            rec[0] = f["n"] | 0x10000 | (raw.size << 17) | (((e >> 32) & 31) << 27)
            rec[1] = e & 0xFFFFFFFF
            rec[2:] = rng.integers(0, 2 ** 32, 18, dtype=np.uint64).astype(np.uint32)      # not defined behind rawlen
            padded = np.concatenate([raw, rng.integers(0, 2, 32 * nw - raw.size, dtype=np.uint8)])
            rec[2:2 + nw] = np.packbits(padded, bitorder="little").view("<u4")
            j += 1
            if not f["good"]:
                k, p, n1, pl = rr.repair(raw)
                if k == 1:
                    want.append((c, e, rr.record(c, e, n1, pl, repaired=True)))
                    want_rep[c] += 1
            if j % 5 == 4:                                  # a record given up before its closing flag
                cand[c, (first[c] + j) % K, 0] = 300 << 17
                cand[c, (first[c] + j) % K, 2:] = 0xFFFFFFFF
                j += 1
        count[c] = j
    assert count.max() <= K and count[:32].sum() > 256 and len(want) > 50        # two passes in block 0
    src, dst = str(tmp_path / "ring.in"), str(tmp_path / "ring.out")
    with open(src, "wb") as f:
        f.write(np.array([N, K, 4096], dtype=np.int32).tobytes() + cand.tobytes() + first.tobytes() + count.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = open(dst, "rb").read()
    flags = np.frombuffer(out[:16], dtype=np.uint32)
    rep = np.frombuffer(out[16:16 + 4 * N], dtype=np.int32)
    fr = np.frombuffer(out[16 + 4 * N:], dtype=FRAME_DTYPE)
    want.sort(key=lambda w: (w[0], w[1]))
    wf = np.zeros(len(want), dtype=FRAME_DTYPE)
    for i, w in enumerate(want):
        wf[i] = w[2]
    stamp = fr["end_bit"].astype(np.int64) | (((fr["flags"].astype(np.int64) >> 1) & 31) << 32)
    assert flags.tolist() == [len(want), 0, 0, 0] and np.array_equal(rep, want_rep)
    assert fr[np.lexsort((stamp, fr["channel"]))].tobytes() == wf.tobytes()


def test_repair_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name
    assert "#define GNUAIS_FRAME_REPAIRED 0x40" in hdr and L.FRAME_REPAIRED == 0x40 == rr.FRAME_REPAIRED


def test_bad_arguments_are_refused_without_a_device(L):
    h = L.load()
    raw = np.zeros(8, dtype=np.uint8)
    pl = np.zeros(53, dtype=np.uint8)
    n, p = C.c_int(), C.c_int()
    out = np.zeros(4, dtype=np.int32)
    assert h.gnuais_repair_candidate(None, 8, pl.ctypes.data, C.byref(n), C.byref(p)) == L.E_ARG
    assert h.gnuais_repair_candidate(raw.ctypes.data, 8, None, C.byref(n), C.byref(p)) == L.E_ARG
    assert h.gnuais_repair_candidate(raw.ctypes.data, 8, pl.ctypes.data, None, C.byref(p)) == L.E_ARG
    assert h.gnuais_repair_candidate(raw.ctypes.data, 8, pl.ctypes.data, C.byref(n), None) == L.E_ARG
    assert h.gnuais_repair_candidate(raw.ctypes.data, -1, pl.ctypes.data, C.byref(n), C.byref(p)) == L.E_ARG
    for on in (0, 1):
        assert h.gnuais_batch_repair(None, on) == L.E_ARG and h.gnuais_node_repair(None, on) == L.E_ARG
    assert h.gnuais_batch_repaired(None, out.ctypes.data) == L.E_ARG
    assert h.gnuais_node_repaired(None, out.ctypes.data) == L.E_ARG


def test_the_kernel_is_built_checked_and_shares_the_trial_with_the_host():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/hdlc_repair.s hdlc_repair_kernel" in mk
    objs = mk.split("OBJS :=")[1].split("\n\n")[0]
    assert "$(BUILD)/hdlc_repair.o" in objs and "$(BUILD)/hdlc_repair_host.o" in objs
    for name in ("hdlc_repair.hip", "hdlc_repair.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "hdlc_repair.h"' in text and "trial_crc(" in text, name
    s_path = os.path.join(CSRC, "build", "hdlc_repair.s")
    assert os.path.exists(s_path), "hdlc_repair.s not built (make -C gnuais_amd/csrc)"
    isa = open(s_path).read()
    assert ".amdhsa_kernel" in isa and "hdlc_repair_kernel" in isa and "gfx950" in isa
