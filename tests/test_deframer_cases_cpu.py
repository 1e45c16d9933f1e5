"""What the inputs of tests/test_deframer_boundaries_gpu.py reach, measured on the CPU restatement alone (no GPU, nothing
the GPU computes): the state protodec_decode() (src/protodec.c:988-1122) is in before every bit of every stream of
tests/deframer_cases.py -- which is the state a split at that bit carries from one decode_bits call into the next -- the
streams' own counters, the pack sizes the GPU tests ask for, and the restatement == the real reference on these streams."""
import numpy as np
import pytest

import deframer_cases as dc
import ref_pins
from oracle_lib import Oracle

ST_SKURR, ST_PREAMBLE, ST_STARTSIGN, ST_DATA, ST_STOPSIGN = 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def carried():
    """{name: [the machine before bit i, for i = 0 .. len (len: after the last bit)]}: one entry per single split"""
    out = {}
    for name in dc.NAMES:
        s = dc.STREAMS[name]
        o = Oracle(1)
        rows = []
        for i in range(s.size + 1):
            rows.append(o.hdlc(0))
            if i < s.size:
                o.decode_bits(0, s[i:i + 1])
        out[name] = rows
    return out


def of_state(carried, state, names=dc.NAMES):
    return [h for n in names for h in carried[n] if h["state"] == state]


def test_streams_are_short_and_one_split_per_position(carried):
    assert max(s.size for s in dc.STREAMS.values()) <= 610
    assert set(dc.STREAMS) == set(dc.COUNTERS)
    n = sum(s.size + 1 for s in dc.STREAMS.values())
    assert len(list(dc.single_splits())) == n == sum(len(r) for r in carried.values())
    assert len(list(dc.double_splits())) == 8 * n
    assert len(list(dc.padded(96))) == 96 * len(dc.NAMES)
    assert len(dc.single_pieces()) == n
    for (name, i, g), p in zip(dc.double_splits(), dc.double_pieces()):
        assert [len(x) for x in p] == [i, min(g, dc.STREAMS[name].size - i), max(0, dc.STREAMS[name].size - i - g)]
        assert np.array_equal(np.concatenate(p), dc.STREAMS[name])
        if i + g > 40:
            break
    (name, p), piece = list(zip(dc.padded(64), dc.padded_pieces(64)))[63]
    assert p == 63 and not piece[0][:63].any() and np.array_equal(piece[0][63:], dc.STREAMS[name])


def test_hunting_is_cut_at_every_count(carried):
    assert {h["antallpreamble"] for h in of_state(carried, ST_SKURR)} == set(range(16))


def test_training_and_flag_are_cut_at_every_count(carried):
    pre = of_state(carried, ST_PREAMBLE)
    assert {h["nstartsign"] for h in pre} >= set(range(6))
    assert {h["antallpreamble"] for h in pre} >= set(range(10))
    assert {h["nstartsign"] for h in of_state(carried, ST_STARTSIGN)} >= {6, 7}
    assert of_state(carried, ST_STOPSIGN)


def test_frames_are_cut_in_every_stuffing_state(carried):
    got = {(h["antallenner"], h["bitstuff"], h["last"]) for h in of_state(carried, ST_DATA)}
    assert got >= {(0, 0, 0), (0, 0, 1), (1, 0, 1), (2, 0, 1), (3, 0, 1), (0, 1, 1)}
    for name in ("over55", "ff55"):                      # a split just before the bit that brings bufferpos to 449
        assert any(h["bufferpos"] == 448 for h in of_state(carried, ST_DATA, [name])), name


def test_the_quirk_states_are_cut_too(carried):
    """a reset in ST_STARTSIGN leaves nstartsign = 1 behind (its trailing ++, protodec.c:1091): ST_SKURR carries it, and
    ST_PREAMBLE is then entered with it"""
    assert any(h["nstartsign"] == 1 for h in of_state(carried, ST_SKURR, ["seven_ones"]))
    assert any(h["nstartsign"] in (1, 2) and h["antallpreamble"] == 0 for h in of_state(carried, ST_PREAMBLE, ["seven_ones"]))


@pytest.mark.parametrize("name", dc.NAMES)
def test_stream_counters(name):
    o = Oracle(1)
    o.decode_bits(0, dc.STREAMS[name])
    assert o.counters()[0].tolist() == dc.COUNTERS[name]


def test_pack_sizes_of_the_increments_the_gpu_tests_use():
    """gnuais_batch_create()'s seg_words, restated once (deframer_cases.pack_words); the GPU tests assert
    info("pack_bits") against the same figures"""
    assert dc.pack_words(1) * 32 == 64
    assert dc.pack_words(934) * 32 == 96
    assert dc.pack_words(0x10000 // 5) * 32 == 480 == dc.pack_words(0) * 32
    assert dc.pack_words(14426) * 32 == 512
    assert dc.PACK_BITS == {1: 64, 934: 96, 0: 480, 14426: 512}
    # the ends of the ranges: 2 words up to 933, 16 from 13463 on, 17 (refused by create) behind 14426
    assert (dc.pack_words(933), dc.pack_words(13462), dc.pack_words(13463), dc.pack_words(14427)) == (2, 15, 16, 17)


def test_restatement_equals_reference_on_these_streams():
    want = ref_pins.want("deframer_boundaries")
    for name in dc.NAMES:
        o = Oracle(1)
        o.decode_bits(0, dc.STREAMS[name])
        assert want["frames_" + name].tobytes() == o.frames().tobytes(), name
        assert np.array_equal(want["counters_" + name], o.counters()), name
        h = o.hdlc(0)
        assert [h[k] for k in ref_pins.FSM] == want["fsm_" + name].tolist(), name
