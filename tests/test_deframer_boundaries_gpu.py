"""The deframer's hand-over between bit packs (hdlc_events.hip, and hdlc_deframe_kernel in hdlc_crc.hip), at every pack
boundary and every pack size: the streams of tests/deframer_cases.py cut at EVERY position, one channel per cut, fed to
gnuais_batch_decode_bits() in two or three calls -- or in one, behind 0 .. pack_bits-1 zeros -- with packs of 64, 96, 480
and 512 bits.  After every call the state machine, the counters and the stored bits of the frames in progress equal the
CPU restatement's, at the end the frames do, end_bit included: bit-exact, no tolerance anywhere.  What the cuts carry
across a boundary is measured in tests/test_deframer_cases_cpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

import deframer_cases as dc
from chain_parity import FSM_KEYS, batch, oracle_fsm_rows
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("receivedframes", "lostframes", "lostframes2")
EMPTY = np.zeros(0, dtype=np.uint8)


def ragged(pieces, labels):
    """+ channels that are fed nothing, until the count is no multiple of 16 or 24 (so of no workgroup width used here
    but 1): the last workgroup has lanes without a channel, and lanes with a channel and without a bit"""
    pieces, labels = list(pieces), list(labels)
    while True:
        pieces.append([EMPTY] * len(pieces[0]))
        labels.append("idle")
        if len(pieces) % 16 and len(pieces) % 24:
            return pieces, labels


@functools.lru_cache(maxsize=None)
def plan(kind, pack_bits=0):
    """(pieces per channel, a label per channel, the restatement's answers): computed once, shared by the cases"""
    if kind == "single":
        pieces, labels = dc.single_pieces(), list(dc.single_splits())
    elif kind == "double":
        pieces, labels = dc.double_pieces(), list(dc.double_splits())
    else:
        pieces, labels = dc.padded_pieces(pack_bits), list(dc.padded(pack_bits))
    pieces, labels = ragged(pieces, labels)
    n = len(pieces)
    o = Oracle(n)
    steps = []
    for k in range(len(pieces[0])):
        for c in range(n):
            o.decode_bits(c, pieces[c][k])
        rows = np.array(oracle_fsm_rows(o, n), dtype=np.int64)
        inside = np.flatnonzero((rows[:, 0] == 4) | (rows[:, 0] == 5))       # ST_DATA, ST_STOPSIGN
        pick = inside[::max(1, -(-inside.size // 200))]                      # <= 200 of them, at a fixed stride
        steps.append((rows, o.counters().copy(), {int(c): o.frame_cells(int(c)) for c in pick}))
    return pieces, labels, steps, o.frames()


def same(got, want, labels, what, call):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    assert bad.size == 0, "%s differ after call %d on %d channels; first: %s" % (
        what, call, bad.size, [(labels[c], np.asarray(got)[c].tolist(), np.asarray(want)[c].tolist()) for c in bad[:5]])


def feed_and_compare(kind, pack_bits, max_len, variant, lpw=0, plan_pack=0):
    pieces, labels, steps, frames = plan(kind, plan_pack)
    n = len(pieces)
    b = batch(n, pllinc=dc.PLLINC_OF_PACK[pack_bits], max_len=max_len)
    assert b.info("pack_bits") == pack_bits == dc.pack_words(dc.PLLINC_OF_PACK[pack_bits]) * 32
    b.set_option("hdlc_variant", variant)
    if lpw:
        b.set_option("hdlc_lpw", lpw)
        assert n % lpw or lpw == 1
    for k, (rows, counters, cells) in enumerate(steps):
        b.decode_bits([p[k] for p in pieces])
        f = b.fsm_state()
        same(np.stack([f[key] for key in FSM_KEYS], axis=1), rows, labels, "state machines", k)
        cnt = b.counters()
        same(np.stack([cnt[key] for key in COUNTER_KEYS], axis=1), counters, labels, "counters", k)
        assert len(cells) >= 100 or k + 1 == len(steps)          # (whole streams end outside a frame)
        for c, want in cells.items():
            got = b.frame_bits(c)
            assert got is not None and np.array_equal(got, want), ("frame cells", k, labels[c])
    assert b.drain_frames().tobytes() == frames.tobytes()
    b.close()


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pack_bits,lpw", [(64, 1), (64, 16), (64, 24), (64, 64), (96, 16), (480, 16), (512, 16)])
def test_every_single_split(pack_bits, lpw, variant):
    """s[:i] in one call, s[i:] in the next, for every i.  At 64 bits a launch is one pack (max_len 2048): every pack
    boundary is a launch boundary too, and the state goes through ctl.  lpw 24 takes the event-driven kernel whose LDS
    offsets are computed, 8 / 16 / 32 / 64 the forms with immediates; 512 bits fill the pack's 16 words."""
    feed_and_compare("single", pack_bits, 2048 if pack_bits == 64 else 48000, variant, lpw)


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pack_bits", [64, 512])
def test_every_split_around_a_short_pack(pack_bits, variant):
    """s[:i], s[i:i+g], s[i+g:] for every i and g = 1 .. 8: the middle call is a pack shorter than 8 bits, which finds the
    1s counted so far in the word before the pack"""
    feed_and_compare("double", pack_bits, 2048, variant, 64)


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pack_bits", [64, 96, 512])
def test_every_offset_inside_a_launch(pack_bits, variant):
    """zeros(p) + s for every p below the pack size, in ONE call of three packs per launch: every position of every
    stream meets a pack boundary inside a launch (the next pack prefetched, the bits counted from pack to pack) and,
    at every third pack, a launch boundary"""
    feed_and_compare("padded", pack_bits, 3 * 2048, variant, plan_pack=pack_bits)


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pllinc", [0, 14426, 1])
def test_a_launch_full_of_the_densest_frames(pllinc, variant):
    """16 alternating bits, a flag, a flag: a frame opened every 32 bits, as fast as the machine allows, for two whole
    decode_bits launches -- more than a run() call of max_len samples can slice.  Every one is counted (lostframes2), the
    drain succeeds and is empty; a second channel's candidates (30 data bits per cycle: lostframes) all reach the CRC."""
    flag = dc.FLAG
    alt = (np.arange(16) & 1).astype(np.uint8)
    b = batch(2, pllinc=pllinc, max_len=48000)
    b.set_option("hdlc_variant", variant)
    pack_bits, segments = int(b.info("pack_bits")), int(b.info("segments"))
    assert pack_bits == dc.PACK_BITS[pllinc] and segments == 24
    cycles = 2 * pack_bits * segments // 32
    data = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.uint8)
    reps = cycles * 32 // 62
    streams = [np.tile(np.concatenate([alt, flag, flag]), cycles), np.tile(np.concatenate([alt, flag, data, flag]), reps)]
    assert streams[0].size == 2 * pack_bits * segments
    o = Oracle(2)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    assert o.counters().tolist() == [[0, 0, cycles], [0, reps, 0]] and len(o.frames()) == 0
    b.decode_bits(streams)
    cnt = b.counters()
    assert np.stack([cnt[key] for key in COUNTER_KEYS], axis=1).tolist() == o.counters().tolist()
    f = b.fsm_state()
    assert np.stack([f[key] for key in FSM_KEYS], axis=1).tolist() == oracle_fsm_rows(o, 2)
    assert len(b.drain_frames()) == 0            # raises GNUAIS_E_OVERFLOW if a candidate found no slot
    b.close()


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pllinc", [1, 14426])
def test_randomised_streams_in_the_smallest_and_the_largest_packs(pllinc, variant):
    """scripts/fuzz_parity.py's deframer case -- adversarial streams cut at random piece sizes -- in 64-bit and in 512-bit
    packs, on both deframers"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
    import fuzz_parity
    for seed in range(2100, 2106):
        res = fuzz_parity.deframer_case(seed, pllinc=pllinc, hdlc_variant=variant)
        assert res.startswith("ok"), (seed, res)
