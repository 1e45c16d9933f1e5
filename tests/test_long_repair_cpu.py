"""Repair of long frames, CPU side: gnuais_long_repair_candidate -- the host's use of the trial text the kernel runs
(gnuais_amd/csrc/hdlc_repair.h with LongLimits) -- against the bit-by-bit restatement (tests/long_repair_ref.py) in
count, position, nbits and payload; the limits; junk; the two cases that keep it apart from the chain's repair; the
ambiguous fixtures; the host unit by itself and both kernels' own text under ASan + UBSan; symbols and argument checks.
No device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hip_cpu_build
import long_ref as lr
import long_repair_ref as lrr
import repair_ref as rr
from gnuais_amd import synth
from test_long_cpu import fields_of, pack_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
NEW_SYMBOLS = ("gnuais_batch_long_repair", "gnuais_batch_long_repaired", "gnuais_long_repair_candidate",
               "gnuais_node_long_repair", "gnuais_node_long_repaired")
flipped = lrr.flipped


@pytest.fixture(scope="module")
def L():
    from gnuais_amd import lib
    return lib


def host_repair(L, raw):
    """gnuais_long_repair_candidate -> (count, p, n', payload bytes) shaped like long_repair_ref.repair()"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    pl = np.full(126, 0xA5, dtype=np.uint8)
    n, p = C.c_int(-7), C.c_int(-7)
    k = L.load().gnuais_long_repair_candidate(raw.ctypes.data, int(raw.size), pl.ctypes.data, C.byref(n), C.byref(p))
    if k != 1:
        assert (n.value, p.value) == (-7, -7) and np.all(pl == 0xA5), "outputs written without a unique trial"
        return (k, None, None, None)
    assert not pl[n.value // 8:].any(), "payload not zero behind nbits / 8 bytes"
    return (1, p.value, n.value, pl[: n.value // 8].tobytes())


def short_host_repair(L, raw):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    pl = np.zeros(53, dtype=np.uint8)
    n, p = C.c_int(-7), C.c_int(-7)
    k = L.load().gnuais_repair_candidate(raw.ctypes.data, int(raw.size), pl.ctypes.data, C.byref(n), C.byref(p))
    return (1, p.value, n.value, pl[: n.value // 8].tobytes()) if k == 1 else (k, None, None, None)


def assert_host_equals_ref(L, raws, what):
    want = lrr.repairs(raws)
    for i, (r, w) in enumerate(zip(raws, want)):
        assert host_repair(L, r) == w, (what, i, len(r))
    return want


@pytest.mark.parametrize("nbytes", [54, 80, 100, 126, 127])
def test_valid_frames_with_one_pair_inverted_at_every_position(L, nbytes):
    """a pair inverted at every p is repaired to the frame, at p, unless another trial passes too (then host and
    restatement agree on the count).  127 bytes are 1016 bits: the trial that undoes the error has n' > 1008, so the
    frame is never repaired into a delivery"""
    payload = bytes(np.random.default_rng(100 + nbytes).integers(0, 256, nbytes, dtype=np.uint8))
    raw = lrr.candidate_raw(payload)
    got = assert_host_equals_ref(L, [flipped(raw, p) for p in range(raw.size - 1)], ("every p", nbytes))
    for p, g in enumerate(got):
        if nbytes == 127:
            assert g[0] == 0 or g[2] <= lr.LONG_MAX_BITS, p
        else:
            assert g[0] >= 1, p                                    # the trial that undoes the error always passes
            if g[0] == 1:
                assert g[1:] == (p, 8 * nbytes, payload), p
    if nbytes == 127:
        assert sum(g[0] for g in got) <= 2                         # what passes here passes by the accident rate alone
    print(f"{nbytes * 8}-bit frame: {len(got)} records, {sum(g[0] == 1 for g in got)} repaired")


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
    raw = np.array(raw + [0, 1, 1, 1, 1, 1], dtype=np.uint8)
    assert np.array_equal(raw, lrr.candidate_raw(payload))
    return raw, where


def crafted(nbytes, seed):
    """a payload with a stuffed zero at a known place (0x1f) and four 1s, a 0 and a 1 at another (0x2f)"""
    payload = bytearray(np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8))
    payload[5:8] = bytes([0x00, 0x1F, 0x00])        # 0 11111 (0) 000: a stuffed zero in the frame
    payload[10:13] = bytes([0x00, 0x2F, 0x00])      # 0 1111 0 1 00
    payload = bytes(payload)
    raw, where = stuffed_with_map(payload)
    a = where[6 * 8 + 4]                            # the fifth 1 of 0x1f; raw[a + 1] is the stuffed zero
    assert raw[a - 4:a + 3].tolist() == [1, 1, 1, 1, 1, 0, 0]
    b = where[11 * 8 + 4]                           # the 0 of 1111 0 1
    assert raw[b - 4:b + 2].tolist() == [1, 1, 1, 1, 0, 1]
    return payload, raw, a, b


@pytest.mark.parametrize("nbytes", [54, 126])
def test_pairs_that_change_the_stuffing_and_pairs_at_the_edges(L, nbytes):
    payload, raw, a, b = crafted(nbytes, 7 + nbytes)
    last = raw.size - 2
    cases = {"destroyed": flipped(raw, a), "made": flipped(raw, b), "six 1s as received": flipped(raw, a + 1),
             "untouched": raw, "flag's 0": flipped(raw, raw.size - 6)}
    edges = (0, 30, 31, 32, 62, 63, 64, last - 1, last)
    cases.update({f"p = {p}": flipped(raw, p) for p in edges})
    by_name = dict(zip(cases, assert_host_equals_ref(L, list(cases.values()), "edges")))
    assert by_name["destroyed"] == (1, a, 8 * nbytes, payload)     # the error destroyed a stuffed zero, the trial makes one
    assert by_name["made"] == (1, b, 8 * nbytes, payload)          # the error made one, the trial destroys it
    assert by_name["six 1s as received"] == (1, a + 1, 8 * nbytes, payload)
    for p in edges:
        g = by_name[f"p = {p}"]
        assert g[0] >= 1 and (g[0] > 1 or g[1:] == (p, 8 * nbytes, payload)), p
    assert by_name["untouched"][0] == 0             # no pair keeps a valid frame valid


def test_the_longest_record_the_stored_limit_and_one_bit_more(L):
    payload = b"\xff" * 126                         # 1008 bits, a stuffed zero behind every five 1s: the longest record
    raw = lrr.candidate_raw(payload)
    assert 1225 <= raw.size <= lrr.REC_RAW == 1236  # 1231: the FCS of this payload has zeros of its own
    ps = sorted(set(range(0, raw.size - 1, 41)) | {31, 63, raw.size - 2, raw.size - 3, raw.size - 7})
    got = assert_host_equals_ref(L, [flipped(raw, p) for p in ps], "longest")
    assert sum(g[0] == 1 and g[3] == payload for g in got) >= len(ps) // 2
    # 1030 stored bits without stuffing: a frame of 1008 bits at the limit is repaired; with one stored bit more
    # bufferpos reaches 1031 and nothing is well formed
    rng = np.random.default_rng(12)
    while True:
        p126 = bytes(rng.integers(0, 256, 126, dtype=np.uint8) & 0x77)     # no run of five 1s inside a byte pair
        r = lrr.candidate_raw(p126)
        if r.size == 1030:
            break
    want = assert_host_equals_ref(L, [flipped(r, 500), flipped(r, 1028)], "at the limit")
    assert want[0] == (1, 500, 1008, p126)
    over = np.concatenate([np.tile(np.array([1, 0], dtype=np.uint8), 512), [0, 1, 0, 1, 1, 1, 1, 1]])
    assert over.size == 1032
    got = assert_host_equals_ref(L, [over, flipped(over, 10), over[1:], np.concatenate([[0] * 7, over])], "over the limit")
    assert [g[0] for g in got[:2]] == [0, 0]


def junk_of(rng, n):
    r = rng.integers(0, 2, n, dtype=np.uint8)
    r[-6:] = [0, 1, 1, 1, 1, 1][-min(n, 6):]
    return r


def test_junk_of_every_length_and_more_than_a_record_holds(L):
    rng = np.random.default_rng(5)
    junk = [junk_of(rng, n) for n in range(2, lrr.MAX_RAW + 1)]
    got = assert_host_equals_ref(L, junk, "junk")
    assert sum(g[0] for g in got) <= 8              # a junk trial passes by the accident rate alone
    assert host_repair(L, np.zeros(lrr.MAX_RAW + 1, dtype=np.uint8))[0] == 0       # 1281: refused, nothing is tried
    assert host_repair(L, junk_of(rng, lrr.MAX_RAW + 1))[0] == 0
    assert host_repair(L, np.zeros(1, dtype=np.uint8))[0] == 0 and host_repair(L, np.zeros(0, dtype=np.uint8))[0] == 0


def test_single_bit_flips_and_two_symbol_errors_are_not_repaired_but_by_accident(L):
    rng = np.random.default_rng(21)
    recs, kinds = [], []
    for nbytes in (54, 126):
        for _ in range(24):
            raw = lrr.candidate_raw(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)))
            one = raw.copy()
            one[int(rng.integers(0, raw.size - 6))] ^= 1
            p, q = sorted(int(v) for v in rng.choice(raw.size - 8, 2, replace=False))
            recs += [one, flipped(flipped(raw, p), q + 2 if q - p < 2 else q)]
            kinds += ["bit", "two"]
    got = assert_host_equals_ref(L, recs, "not single symbol errors")
    # against the restatement, not against zero: at most 1235 / 65536 of them are accepted wrongly
    assert sum(g[0] == 1 for g in got) <= 6


def test_the_two_repairs_are_disjoint(L):
    """n' > 426 keeps them apart.  A 424-bit frame with a symbol error that destroyed a stuffed zero is the chain's: its
    one passing trial has n' = 424, which the long repair does not take.  A 432-bit frame whose error made a stuffed zero
    has n = 431 in D'; the chain's decoder gave it up at 449 stored bits, the long repair delivers it"""
    p53, raw53, a, _ = crafted(53, 60)
    rec = flipped(raw53, a)
    assert rr.repair(rec) == short_host_repair(L, rec) == (1, a, 424, p53)
    assert lrr.repair(rec) == host_repair(L, rec) == (0, None, None, None)
    assert lrr.repair(rec, limit=449, min_bits=0) == (1, a, 424, p53)      # the same restatement with the chain's numbers
    p54, raw54, _, b = crafted(54, 61)
    rec = flipped(raw54, b)
    d = lrr.RawLongDeframer()
    d.feed(np.concatenate([synth.hdlc_frame_bits(p54)[:32], rec, [1, 0]]))
    assert [(f["n"], f["good"]) for f in d.closed] == [(431, False)] and np.array_equal(d.closed[0]["raw"], rec)
    assert lrr.repair(rec) == host_repair(L, rec) == (1, b, 432, p54)
    assert rr.repair(rec)[0] == 0 and short_host_repair(L, rec)[0] == 0


def ambiguous_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "long_repair_ambiguous.json")) as f:
        return json.load(f)


def test_candidates_that_two_trials_repair_stay_lost(L):
    fixtures = ambiguous_fixtures()
    assert len(fixtures) >= 2
    for fx in fixtures:
        raw = flipped(lrr.candidate_raw(bytes.fromhex(fx["payload"])), fx["p1"])
        passing = lrr.brute_force(raw)
        assert [t[0] for t in passing] == fx["passes_at"] and len(passing) == 2 and fx["p1"] in fx["passes_at"], fx
        assert passing[0][2] != passing[1][2]                      # two different frames, both with a good CRC
        assert host_repair(L, raw) == (2, None, None, None), fx


SAN_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "gnuais_hip.h"
/* argv: in out; in: records of (int32 n_raw, n_raw bytes); out: per record int32 count, p, nbits + 126 payload bytes */
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 3;
    int32_t n;
    while (fread(&n, sizeof n, 1, f) == 1) {
        uint8_t *exact = malloc((size_t) n ? (size_t) n : 1);      /* exactly n bytes are the record's */
        if (n && fread(exact, 1, (size_t) n, f) != (size_t) n) return 4;
        uint8_t *payload = malloc(126);
        for (int i = 0; i < 126; ++i) payload[i] = 0xA5;
        int nbits = -7, pos = -7;
        const int32_t k = gnuais_long_repair_candidate(exact, n, payload, &nbits, &pos);
        const int32_t head[3] = {k, pos, nbits};
        if (fwrite(head, sizeof head, 1, g) != 1 || fwrite(payload, 1, 126, g) != 126) return 5;
        free(exact);
        free(payload);
    }
    uint8_t none[126];
    int a = 0, b = 0;
    if (gnuais_long_repair_candidate(NULL, 5, none, &a, &b) != GNUAIS_E_ARG) return 6;
    fclose(f);
    fclose(g);
    return 0;
}
'''


def test_long_repair_candidate_standalone_under_asan_and_ubsan(L, tmp_path):
    """hdlc_long_repair.cpp has no HIP dependency: g++ builds it by itself with -fsanitize=address,undefined, and records
    of the edge cases, the limits, junk of every length and the ambiguous fixtures give what the library gives"""
    exe = str(tmp_path / "long_repair.bin")
    main_c = tmp_path / "main.c"
    main_c.write_text(SAN_MAIN)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-c",
                           str(main_c), "-o", str(tmp_path / "main.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *san, "-c", os.path.join(CSRC, "hdlc_long_repair.cpp"),
                           "-o", str(tmp_path / "hdlc_long_repair.o")])
    subprocess.check_call(["g++", *san, str(tmp_path / "main.o"), str(tmp_path / "hdlc_long_repair.o"), "-o", exe])
    rng = np.random.default_rng(9)
    recs = []
    for nbytes in (54, 126, 127):
        raw = lrr.candidate_raw(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)))
        recs += [flipped(raw, p) for p in range(0, raw.size - 1, 7)] + [flipped(raw, raw.size - 2)]
    full = lrr.candidate_raw(b"\xff" * 126)
    recs += [flipped(full, p) for p in (0, 31, 63, full.size - 2)]
    recs += [flipped(lrr.candidate_raw(bytes.fromhex(fx["payload"])), fx["p1"]) for fx in ambiguous_fixtures()]
    for n in list(range(0, lrr.MAX_RAW + 2)) + [4000]:
        recs.append(junk_of(rng, n) if n >= 6 else rng.integers(0, 2, n, dtype=np.uint8))
    recs.append(np.ones(lrr.MAX_RAW, dtype=np.uint8))
    src, dst = str(tmp_path / "records.in"), str(tmp_path / "records.out")
    with open(src, "wb") as f:
        for r in recs:
            f.write(np.int32(r.size).tobytes() + r.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = np.fromfile(dst, dtype=np.dtype([("head", "<i4", (3,)), ("payload", "u1", (126,))]))
    assert out.size == len(recs)
    for rec, o in zip(recs, out):
        k, p, n, payload = host_repair(L, rec)
        if k == 1:
            assert o["head"].tolist() == [1, p, n] and o["payload"][: n // 8].tobytes() == payload
        else:
            assert o["head"].tolist() == [k, -7, -7] and np.all(o["payload"] == 0xA5)


# ---- both kernels' own text on the CPU --------------------------------------------------------------------------------
def test_both_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path):
    """hdlc_long.hip in its form that keeps the raw bits and hdlc_long_repair.hip compiled for the CPU behind
    tests/c/hip_cpu (a thread per lane, a block of 64 at a time) under ASan + UBSan and run through their launch
    functions: 70 channels over three calls that cut the bursts, so candidates straddle calls, with stamps above 2^32 and
    the repair on three workgroups: records, the three counters and the carried state after every call are the
    restatement's."""
    exe = hip_cpu_build.build("long_repair_kernel_main.cpp", tmp_path / "long_repair_kernel.bin")
    N, n_seg, seg_words, cap, cand_cap, blocks = 70, 16, 15, 512, 512, 3
    rng = np.random.default_rng(32)
    streams = [lrr.damaged_channel_bits(rng, c) for c in range(N)]
    seen0 = np.array([(1 << 32) - 700 + 13 * c if c % 2 else (5 << 32) + (1 << 31) + c for c in range(N)], dtype=np.uint64)
    seen0[3] = (1 << 37) - 900                  # the stamp wraps inside this channel's stream
    lens = (n_seg * 2048, n_seg * 2048 - 5, n_seg * 2048 - 77)
    n0 = (1 << 31) - 5000
    cuts = [sorted(int(v) for v in rng.integers(200, s.size - 200, 2)) for s in streams]
    pieces = [[s[:k[0]] for s, k in zip(streams, cuts)], [s[k[0]:k[1]] for s, k in zip(streams, cuts)],
              [s[k[1]:] for s, k in zip(streams, cuts)]]
    calls = pack_calls(pieces, n_seg, seg_words)
    src, dst = str(tmp_path / "long.in"), str(tmp_path / "long.out")
    with open(src, "wb") as f:
        f.write(np.array([N, n_seg, seg_words, cap, len(calls), cand_cap, blocks], dtype=np.int64).tobytes() + seen0.tobytes())
        row = n0
        for (words, cnt), ln in zip(calls, lens):
            f.write(np.array([ln, row], dtype=np.int64).tobytes() + words.tobytes() + cnt.tobytes())
            row += ln
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    raw = open(dst, "rb").read()
    per_call = np.frombuffer(raw, dtype="<u4", count=3 * (3 * N + 1)).reshape(3, 3 * N + 1)
    lctl, listed = per_call[:, :3 * N].reshape(3, 3, N), per_call[:, 3 * N]
    off = per_call.nbytes
    counters = np.frombuffer(raw, dtype="<i4", count=3 * N, offset=off).reshape(3, N)
    count = np.frombuffer(raw, dtype="<u4", count=2, offset=off + counters.nbytes)
    got = np.frombuffer(raw, dtype=lr.LONG_FRAME_DTYPE, offset=off + counters.nbytes + 8)

    pack = seg_words * 32
    where = {}
    states = []
    for c in range(N):
        d = lr.LongDeframer(seen=int(seen0[c]))
        row, base = n0, 0
        for k, ln in enumerate(lens):
            part = pieces[k][c]
            d.feed(part)
            assert fields_of(lctl[k, 0, c]) == d.fields(), (c, k)
            for f in d.closed:
                if base <= f["index"] < base + len(part):
                    s, jj = divmod(f["index"] - base, pack)
                    c_s = min(pack, len(part) - s * pack)
                    l_s = min(2048, ln - s * 2048)
                    where[c, f["end_bit"]] = row + s * 2048 + ((2 * jj + 1) * l_s) // (2 * c_s)
            base += len(part)
            row += ln
        states.append(d)
    want, want_counters, ds = lrr.decode_streams(streams, seen=seen0, times=lambda c, f: where[c, f["end_bit"]])
    assert count[1] == 0 and count[0] == len(want) == got.size
    order = np.lexsort((got["end_bit"].astype(np.uint64) | ((got["flags"].astype(np.uint64) >> 1 & 31) << 32), got["channel"]))
    assert got[order].tobytes() == want.tobytes()
    assert np.array_equal(counters.T, want_counters)
    assert int(listed.sum()) == int(want_counters[:, 1].sum())          # every failed frame was listed, in its call
    repaired = want[(want["flags"] & rr.FRAME_REPAIRED) != 0]
    assert len(repaired) > 20 and want_counters[:, 1].sum() > len(repaired) + 20 and len(want) - len(repaired) > 20
    assert (repaired["flags"] >> 1 & 31).max() >= 5 and repaired["t"].max() > 1 << 31
    assert {int(n) for n in repaired["nbits"]} >= {432, 480, 800, 1008} and 1016 not in want["nbits"]
    # candidates that straddle calls: a repaired frame that closed in a later call than it started in
    ends = {(int(r["channel"]), int(r["end_bit"])) for r in repaired}
    straddle = 0
    for c, d in enumerate(ds):
        for f in d.candidates():
            if (c, f["end_bit"] & 0xFFFFFFFF) in ends:
                start = f["index"] - len(f["raw"])
                straddle += any(start < k <= f["index"] for k in cuts[c])
    assert straddle >= 3


def test_long_repair_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr, name
        assert name in L.SYMBOLS, name
        assert getattr(handle, name).argtypes == L.SYMBOLS[name][1], name
    from gnuais_amd.receiver import ReceiverBatch
    from gnuais_amd.shard import ReceiverNode
    for cls in (ReceiverBatch, ReceiverNode):
        assert callable(getattr(cls, "long_repair")) and callable(getattr(cls, "long_repaired"))


def test_bad_arguments_are_refused_without_a_device(L):
    h = L.load()
    raw = np.zeros(8, dtype=np.uint8)
    pl = np.zeros(126, dtype=np.uint8)
    n, p = C.c_int(), C.c_int()
    out = np.zeros(4, dtype=np.int32)
    assert h.gnuais_long_repair_candidate(None, 8, pl.ctypes.data, C.byref(n), C.byref(p)) == L.E_ARG
    assert h.gnuais_long_repair_candidate(raw.ctypes.data, 8, None, C.byref(n), C.byref(p)) == L.E_ARG
    assert h.gnuais_long_repair_candidate(raw.ctypes.data, 8, pl.ctypes.data, None, C.byref(p)) == L.E_ARG
    assert h.gnuais_long_repair_candidate(raw.ctypes.data, 8, pl.ctypes.data, C.byref(n), None) == L.E_ARG
    assert h.gnuais_long_repair_candidate(raw.ctypes.data, -1, pl.ctypes.data, C.byref(n), C.byref(p)) == L.E_ARG
    for on in (0, 1):
        assert h.gnuais_batch_long_repair(None, on) == L.E_ARG and h.gnuais_node_long_repair(None, on) == L.E_ARG
    assert h.gnuais_batch_long_repaired(None, out.ctypes.data) == L.E_ARG
    assert h.gnuais_node_long_repaired(None, out.ctypes.data) == L.E_ARG


def test_the_formatter_takes_a_repaired_record_as_any_other():
    """gnuais_nmea_from_long_frames does not look at flags: bit 6 set or clear, the sentences are the same"""
    from gnuais_amd.receiver import nmea_from_long_frames
    from test_long_cpu import long_records, with_type
    rng = np.random.default_rng(8)
    items = [(0, 1008, with_type(rng, 126, 8)), (1, 432, with_type(rng, 54, 6)), (0, 800, with_type(rng, 100, 12))]
    plain = long_records(items)
    marked = plain.copy()
    marked["flags"] |= rr.FRAME_REPAIRED
    s1, s2 = np.array([0, 7], dtype=np.uint8), np.array([0, 7], dtype=np.uint8)
    a, b = nmea_from_long_frames(plain, s1), nmea_from_long_frames(marked, s2)
    assert a == b and a.count(b"!AIVDM") >= 7 and s1.tolist() == s2.tolist()


def test_the_kernels_are_built_checked_and_share_the_trial_with_the_host():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/hdlc_long_repair.s hdlc_long_repair_kernel" in mk
    assert "$(CHECK_RES) $(BUILD)/hdlc_repair.s hdlc_repair_kernel" in mk and "$(CHECK_RES) $(BUILD)/hdlc_long.s hdlc_long_kernel" in mk
    objs = mk.split("OBJS :=")[1].split("\n\n")[0]
    assert "$(BUILD)/hdlc_long_repair.o" in objs and "$(BUILD)/hdlc_long_repair_host.o" in objs
    for name in ("hdlc_long_repair.hip", "hdlc_long_repair.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "hdlc_repair.h"' in text and "trial_crc<" in text and "LongLimits" in text, name
    for s_name, kernels in (("hdlc_long_repair.s", ("hdlc_long_repair_kernel",)),
                            ("hdlc_long.s", ("hdlc_long_kernelILb0EE", "hdlc_long_kernelILb1EE"))):
        s_path = os.path.join(CSRC, "build", s_name)
        assert os.path.exists(s_path), f"{s_name} not built (make -C gnuais_amd/csrc)"
        isa = open(s_path).read()
        assert ".amdhsa_kernel" in isa and "gfx950" in isa and all(k in isa for k in kernels)
