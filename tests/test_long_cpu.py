"""The long-frame decoder D' (include/gnuais_hip.h, gnuais_batch_long_frames) without a GPU: the restatement
tests/long_ref.py against the reference's machine and against what D' must deliver, and hdlc_long.hip's own text on the
CPU under ASan + UBSan against the restatement."""
import os
import subprocess

import numpy as np
import pytest

import deframer_cases as dc
import hip_cpu_build
import long_ref as lr
import repair_ref as rr
from gnuais_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")
SEEDS = (10, 11, 12, 13, 14, 15)        # the noisy inputs of tests/test_repair_cpu.py
SIGMAS = (5000, 6000)
LONG_BYTES = lr.LONG_BYTES


def long_stream(sigma, seed=9):
    return synth.make_stream(6 * 8 * 1280, seed=seed, sigma=float(sigma), payloads=lr.long_payloads())


def assert_same_machine(d, ref, oracle_hdlc, frames, what):
    assert (d.received, d.lost, d.lost2) == (ref.received, ref.lost, ref.lost2), what
    assert [(f["n"], f["good"], f["payload"], f["end_bit"]) for f in d.closed] == \
           [(f["n"], f["good"], f["payload"], f["end_bit"]) for f in ref.closed], what
    assert d.fields() == (ref.state, ref.nstartsign, min(ref.antallpreamble, 15), ref.antallenner, ref.bitstuff, ref.last,
                          ref.bufferpos), what
    h = oracle_hdlc
    assert (d.received, d.lost, d.lost2) == (h["receivedframes"], h["lostframes"], h["lostframes2"]), what
    assert d.fields() == (h["state"], h["nstartsign"], min(h["antallpreamble"], 15), h["antallenner"], h["bitstuff"],
                          h["last"], h["bufferpos"]), what
    good = [f for f in d.closed if f["good"]]
    assert [f["end_bit"] & 0xFFFFFFFF for f in good] == [int(e) for e in frames["end_bit"]], what
    assert [(f["n"], f["payload"]) for f in good] == [(int(f["nbits"]), bytes(f["payload"][: f["nbits"] // 8])) for f in frames], what


def test_with_the_references_limit_the_restatement_is_the_reference():
    """limit 449, buffer 450: frames, stamps, the three counters and the final state of repair_ref.Deframer and of the
    oracle, on every stream of tests/deframer_cases.py and on the noisy inputs of tests/test_repair_cpu.py"""
    from oracle_lib import Oracle
    inputs = [(name, dc.STREAMS[name]) for name in dc.NAMES]
    for sigma in SIGMAS:
        for seed in SEEDS:
            x, _ = synth.make_stream(4 * 48000, seed=seed, amplitude=12000.0, sigma=float(sigma), occupancy=0.5)
            inputs.append(((sigma, seed), Oracle(1).run(x[:, None], want_bits=True)["bits"][0]))
    closed = 0
    for what, bits in inputs:
        d, ref, o = lr.LongDeframer(limit=449, buffer=450), rr.Deframer(), Oracle(1)
        d.feed(bits)
        ref.feed(bits)
        o.decode_bits(0, bits)
        assert_same_machine(d, ref, o.hdlc(0), o.frames(), what)
        closed += len(d.closed)
    assert closed > 500


@pytest.fixture(scope="module")
def long_inputs():
    """per sigma: (placed payloads, the oracle's bits) of the seed-9 stream with the eight long and short bursts"""
    from oracle_lib import Oracle
    out = {}
    for sigma in (500, 3000):
        x, placed = long_stream(sigma)
        out[sigma] = (placed, Oracle(1).run(x[:, None], want_bits=True)["bits"][0], x)
    return out


def test_the_raised_limit_delivers_three_to_five_slots_and_nothing_else(long_inputs):
    from oracle_lib import Oracle
    for sigma, (placed, bits, x) in long_inputs.items():
        assert [len(p) for _, p in placed] == list(LONG_BYTES)
        by_len = {len(p): p for _, p in placed}
        d = lr.LongDeframer()
        d.feed(bits)
        got = d.long_frames()
        assert len(got) == 5, sigma                                  # a generator change cannot empty the test
        assert [f["n"] for f in got] == [432, 480, 640, 800, 1008], sigma
        for f in got:
            assert f["payload"] == by_len[f["n"] // 8], (sigma, f["n"])
        assert all(f["n"] != 127 * 8 for f in d.closed) and all(f["n"] > lr.SHORT_BITS for f in got)
        assert d.long_counters() == (5, 0)
        # the reference's machine on the same bits: the two short frames, frame for frame what the restatement at 449 gives
        ref = lr.LongDeframer(limit=449, buffer=450)
        ref.feed(bits)
        o = Oracle(1)
        o.decode_bits(0, bits)
        assert [(f["n"], f["payload"]) for f in ref.closed if f["good"]] == [(424, by_len[53]), (168, by_len[21])]
        assert [int(f["nbits"]) for f in o.frames()] == [424, 168]
        # and D' walks over those two: same stamps, it just does not deliver them
        assert [f["end_bit"] for f in d.closed if f["n"] <= lr.SHORT_BITS and f["good"]] == [f["end_bit"] for f in ref.closed if f["good"]]


# ---- the kernel's own text on the CPU ---------------------------------------------------------------------------------
def pack_calls(pieces, n_seg, seg_words):
    """pieces[call][channel] = bits -> per call (segbits [N][n_seg][16] u32, segcnt [N][n_seg] u32), packs filled to
    their capacity in order as gnuais_batch_decode_bits fills them"""
    cap = seg_words * 32
    out = []
    for call in pieces:
        N = len(call)
        words = np.zeros((N, n_seg, 16), dtype=np.uint32)
        cnt = np.zeros((N, n_seg), dtype=np.uint32)
        for c, bits in enumerate(call):
            assert len(bits) <= cap * n_seg
            for s in range(n_seg):
                part = np.asarray(bits[s * cap:(s + 1) * cap], dtype=np.uint8)
                cnt[c, s] = part.size
                padded = np.zeros(16 * 32, dtype=np.uint8)
                padded[:part.size] = part
                words[c, s] = np.packbits(padded, bitorder="little").view("<u4")
        out.append((words, cnt))
    return out


def fields_of(word0):
    w = int(word0)
    return (w & 7, (w >> 3) & 15, (w >> 7) & 15, (w >> 11) & 7, (w >> 14) & 1, (w >> 15) & 1, (w >> 16) & 2047)


def test_the_kernels_own_text_on_the_cpu_equals_the_restatement(tmp_path):
    """hdlc_long.hip compiled for the CPU behind tests/c/hip_cpu (a thread per lane, a block of 64 at a time) under ASan +
    UBSan and run through launch_hdlc_long_reset() and launch_hdlc_long(): the bit packs of 70 channels over three calls that cut the bursts -- the middle call a single bit --
    with stamps above 2^32: records, counters and the carried state after every call are the restatement's."""
    exe = hip_cpu_build.build("long_kernel_main.cpp", tmp_path / "long_kernel.bin")
    N, n_seg, seg_words, cap = 70, 16, 15, 512
    rng = np.random.default_rng(31)
    streams = [lr.channel_bits(rng, c) for c in range(N)]
    seen0 = np.array([(1 << 32) - 700 + 13 * c if c % 2 else (5 << 32) + (1 << 31) + c for c in range(N)], dtype=np.uint64)
    seen0[3] = (1 << 37) - 900                  # the stamp wraps inside this channel's stream
    lens = (n_seg * 2048, 1, n_seg * 2048 - 77) # rows of the three calls; the times come from them and the packs
    n0 = (1 << 31) - 5000                       # t crosses 2^31 rows
    cuts = [int(rng.integers(200, s.size - 200)) for s in streams]
    pieces = [[s[:k] for s, k in zip(streams, cuts)], [s[k:k + 1] for s, k in zip(streams, cuts)],
              [s[k + 1:] for s, k in zip(streams, cuts)]]
    calls = pack_calls(pieces, n_seg, seg_words)
    src, dst = str(tmp_path / "long.in"), str(tmp_path / "long.out")
    with open(src, "wb") as f:
        f.write(np.array([N, n_seg, seg_words, cap, len(calls)], dtype=np.int64).tobytes() + seen0.tobytes())
        row = n0
        for (words, cnt), ln in zip(calls, lens):
            f.write(np.array([ln, row], dtype=np.int64).tobytes() + words.tobytes() + cnt.tobytes())
            row += ln
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    raw = open(dst, "rb").read()
    lctl = np.frombuffer(raw, dtype="<u4", count=3 * 3 * N).reshape(3, 3, N)
    off = lctl.nbytes
    counters = np.frombuffer(raw, dtype="<i4", count=2 * N, offset=off).reshape(2, N)
    count = np.frombuffer(raw, dtype="<u4", count=2, offset=off + counters.nbytes)
    got = np.frombuffer(raw, dtype=lr.LONG_FRAME_DTYPE, offset=off + counters.nbytes + 8)

    # the restatement, and where each closing bit lies: call, pack, slice -> the receive time of the definition
    pack = seg_words * 32
    ds = []
    where = {}
    for c in range(N):
        d = lr.LongDeframer(seen=int(seen0[c]))
        row = n0
        base = 0
        for k, ln in enumerate(lens):
            part = pieces[k][c]
            d.feed(part)
            assert fields_of(lctl[k, 0, c]) == d.fields(), (c, k)
            for f in d.closed:
                if base <= f["index"] < base + len(part):
                    j = f["index"] - base
                    s, jj = divmod(j, pack)
                    c_s = min(pack, len(part) - s * pack)
                    l_s = min(2048, ln - s * 2048)
                    where[c, f["end_bit"]] = row + s * 2048 + ((2 * jj + 1) * l_s) // (2 * c_s)
            base += len(part)
            row += ln
        ds.append(d)
    want = lr.records(ds, times=lambda c, f: where[c, f["end_bit"]])
    assert count[1] == 0 and count[0] == len(want) == got.size
    order = np.lexsort((got["end_bit"].astype(np.uint64) | ((got["flags"].astype(np.uint64) >> 1 & 31) << 32), got["channel"]))
    assert got[order].tobytes() == want.tobytes()
    assert np.array_equal(counters.T, np.array([d.long_counters() for d in ds], dtype=np.int32))
    assert len(want) > 100 and counters[1].sum() > 10
    assert (want["flags"] >> 1).max() >= 5 and want["t"].max() > 1 << 31 > want["t"].min()
    assert {int(n) for n in want["nbits"]} >= {432, 440, 480, 800, 1008} and 1016 not in want["nbits"]


# ---- gnuais_nmea_from_long_frames ---------------------------------------------------------------------------------------
def long_records(items):
    """items: (channel, nbits, payload bytes) -> LONG_FRAME_DTYPE records"""
    out = np.zeros(len(items), dtype=lr.LONG_FRAME_DTYPE)
    for r, (c, nbits, payload) in zip(out, items):
        r["channel"], r["nbits"], r["flags"], r["t"] = c, nbits, 1, -1
        r["payload"][: len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    return out


def with_type(rng, nbytes, typ):
    p = bytearray(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())
    p[0] = (typ << 2) | (p[0] & 3)
    return bytes(p)


def test_long_sentences_equal_the_two_reference_functions_restated():
    from gnuais_amd.receiver import nmea_from_long_frames
    rng = np.random.default_rng(5)
    items = []
    for nbytes in range(54, 127):                           # every length; the type from the whole range, 0 and 28 among them
        items.append((nbytes % 3, 8 * nbytes, with_type(rng, nbytes, int(rng.integers(1, 25)))))
    for nbits in (427, 431, 433, 500, 733, 1001, 1003, 1007):   # bit counts that are no multiple of 6, nor of 8
        items.append((1, nbits, with_type(rng, nbits // 8 + 1, 8)))
    for typ in (0, 28, 25, 63):                             # no sentence, the digit does not move
        items.append((2, 800, with_type(rng, 100, typ)))
    items += [(0, 1008, with_type(rng, 126, 6))] * 12      # the digit rolls over 9
    recs = long_records(items)
    seq = np.array([3, 0, 9], dtype=np.uint8)
    want, digits = b"", [3, 0, 9]
    for c, nbits, payload in items:
        s, digits[c] = lr.ref_sentences(payload, nbits, digits[c])
        want += s
    got = nmea_from_long_frames(recs, seq)
    assert got == want and seq.tolist() == digits
    lines = got.split(b"\r\n")[:-1]
    assert max(len(l) for l in lines) == 1 + 13 + 61 + 5 and {l[7:8] for l in lines} == {b"2", b"3"}
    assert sum(1 for it in items if it[2][0] >> 2 in (0, 28, 25, 63)) >= 4 and len(lines) > 200


def test_short_records_in_the_long_struct_give_the_short_formatters_bytes():
    """records of at most 424 bits, which gnuais_nmea_from_frames -- pinned to the reference -- formats too"""
    from gnuais_amd.lib import FRAME_DTYPE
    from gnuais_amd.receiver import nmea_from_frames, nmea_from_long_frames
    rng = np.random.default_rng(6)
    items = [(int(rng.integers(0, 4)), nbits, with_type(rng, nbits // 8, int(rng.integers(0, 30))))
             for nbits in list(range(8, 425, 8)) + [168, 424, 424, 366, 367, 372, 423]]
    short = np.zeros(len(items), dtype=FRAME_DTYPE)
    for r, (c, nbits, payload) in zip(short, items):
        r["channel"], r["nbits"], r["flags"] = c, nbits, 1
        r["payload"][: len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    s1, s2 = np.array([0, 5, 9, 2], dtype=np.uint8), np.array([0, 5, 9, 2], dtype=np.uint8)
    a = nmea_from_frames(short, s1)
    b = nmea_from_long_frames(long_records(items), s2)
    assert a == b and len(a) > 2000 and s1.tolist() == s2.tolist()


def test_long_sentences_sizing_overflow_and_arguments():
    import ctypes as C
    from gnuais_amd import lib
    L = lib.load()
    rng = np.random.default_rng(7)
    recs = long_records([(0, 1008, with_type(rng, 126, 8)), (1, 480, with_type(rng, 60, 6))])
    seq = np.zeros(2, dtype=np.uint8)
    need, ns = C.c_size_t(0), C.c_int(0)
    # sizing: no buffer, the length comes back, the digits move as in a real call (gnuais_nmea_from_frames does the same)
    rc = L.gnuais_nmea_from_long_frames(recs.ctypes.data, 2, seq.ctypes.data, 2, None, 0, C.byref(need), C.byref(ns))
    assert rc == lib.OK and ns.value == 5 and need.value > 5 * 20
    full = np.zeros(need.value, dtype=np.uint8)
    seq[:] = 0
    assert L.gnuais_nmea_from_long_frames(recs.ctypes.data, 2, seq.ctypes.data, 2, full.ctypes.data, full.size, C.byref(need),
                                          C.byref(ns)) == lib.OK and need.value == full.size
    small = np.full(full.size - 1, 0xA5, dtype=np.uint8)
    seq[:] = 0
    n2 = C.c_size_t(0)
    assert L.gnuais_nmea_from_long_frames(recs.ctypes.data, 2, seq.ctypes.data, 2, small.ctypes.data, small.size, C.byref(n2),
                                          C.byref(ns)) == lib.E_OVERFLOW and n2.value == full.size
    for bad in (dict(n=-1), dict(nch=1), dict(nbits=1009), dict(seq=None), dict(need=None)):
        r = recs.copy()
        if "nbits" in bad:
            r["nbits"][0] = bad["nbits"]
        rc = L.gnuais_nmea_from_long_frames(r.ctypes.data, bad.get("n", 2), None if "seq" in bad else seq.ctypes.data,
                                            bad.get("nch", 2), full.ctypes.data, full.size,
                                            None if "need" in bad else C.byref(need), C.byref(ns))
        assert rc == lib.E_ARG, bad


def test_long_symbols_declared_exported_and_the_kernel_is_in_the_builds_resource_check():
    from gnuais_amd import lib
    header = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    for name in ("gnuais_batch_long_frames", "gnuais_batch_pending_long_frames", "gnuais_batch_drain_long_frames",
                 "gnuais_batch_long_counters", "gnuais_batch_long_fsm_state", "gnuais_nmea_from_long_frames",
                 "gnuais_node_long_frames", "gnuais_node_drain_long_frames", "gnuais_node_long_counters"):
        assert name in lib.SYMBOLS and name + "(" in header and hasattr(lib.load(), name)
    assert lib.LONG_FRAME_DTYPE == lr.LONG_FRAME_DTYPE and "} gnuais_long_frame;   /* 152 bytes */" in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(CHECK_RES) $(BUILD)/hdlc_long.s hdlc_long_kernel" in mk
    text = open(os.path.join(CSRC, "hdlc_long.hip")).read()
    assert "hdlc_crc.hip" in text and "#include \"hdlc" not in text      # its own walk: nothing of the chain's kernels is shared
