"""The PLL stage's reference and inputs, on the CPU (no GPU needed).

  * tests/pll_ref.py::pll_run is the reference: at every clock increment of pll_ref.PLLINCS its bits and carried state
    equal the compiled reference's (live from oracle/_ref, or its recorded answers in tests/golden/ref_pins.npz) and
    the restatement's (oracle/ais_oracle.c), which also agree on the deframer's counters, state and frames.
  * the inputs of tests/test_pll_gpu.py do what they are there for.  These conditions are asserted on pll_run's record
    of the slicer's decisions on pll_ref.columns() alone, so that a later change of the inputs cannot hollow the GPU
    tests out.  Figures measured on the reference loop stand beside each floor."""
import functools

import numpy as np
import pytest

import pll_ref
import ref_pins
from oracle_lib import Oracle
from pll_ref import COLUMN_NAMES, PLLINCS

TOTAL = 12000
FAST, SLOW = COLUMN_NAMES.index("fast"), COLUMN_NAMES.index("slow")


@functools.lru_cache(maxsize=None)
def records(pllinc):
    """pll_run on what the slicer decides on every column: [(bits, state, record)] (computed once per increment)"""
    s = pll_ref.signs_of(pll_ref.columns(TOTAL, pllinc))
    return [pll_ref.pll_run(s[:, c], pllinc) for c in range(s.shape[1])]


def test_the_pass_through_table_delays_by_five_samples():
    """signs_of() is the restatement's filter output > 0, sample for sample, over ragged calls"""
    x = pll_ref.columns(3000, 4096)
    o = Oracle(x.shape[1], taps=pll_ref.TAPS, pllinc=4096)
    got = np.concatenate([o.run(x[a:b], want_filtered=True)["filtered"] > 0 for a, b in ((0, 1), (1, 4), (4, 2049), (2049, 3000))])
    assert np.array_equal(got.astype(np.uint8), pll_ref.signs_of(x))
    assert np.array_equal(pll_ref.signs_of(x[100:], history=x[:100]), pll_ref.signs_of(x)[100:])


@pytest.mark.parametrize("pllinc", PLLINCS)
def test_oracle_equals_reference_equals_pll_run(pllinc):
    want = ref_pins.want("pll_%d" % pllinc)
    x = ref_pins.pll_columns(pllinc)
    signs = pll_ref.signs_of(x)
    for j, name in enumerate(ref_pins.PLL_PIN_COLUMNS):
        o = Oracle(1, taps=pll_ref.TAPS, pllinc=pllinc)
        r = o.run(x[:, j:j + 1], want_bits=True)
        bits, state, _ = pll_ref.pll_run(signs[:, j], pllinc)
        assert np.array_equal(want["bits_%d" % j], r["bits"][0]), name
        assert np.array_equal(want["bits_%d" % j], bits), name
        assert tuple(want["pll_%d" % j][0]) == o.pll(0) == state, name
        assert np.array_equal(want["counters_%d" % j], o.counters()), name
        assert want["frames_%d" % j].tobytes() == o.frames().tobytes(), name
        h = o.hdlc(0)
        assert all(h[k] == want["fsm_%d" % j][0][i] for i, k in enumerate(ref_pins.FSM)), name
        # and the same column inside pll_ref.columns() is the same column
        assert np.array_equal(records(pllinc)[COLUMN_NAMES.index(name)][0], bits)


@pytest.mark.parametrize("pllinc", PLLINCS)
def test_pll_run_carries_its_state_across_ragged_calls(pllinc):
    s = pll_ref.signs_of(pll_ref.columns(TOTAL, pllinc))[:, COLUMN_NAMES.index("fast_slow_3000")]
    chunks = (4097, 255, 1, 2048, 256, 257, 3086)             # the ragged calls of tests/test_pll_gpu.py
    bits, state, rec = pll_ref.pll_run(s[:sum(chunks)], pllinc)
    got, st, pos, rows = [], None, 0, []
    for n in chunks:
        b, st, r = pll_ref.pll_run(s[pos:pos + n], pllinc, st)
        got.append(b)
        rows.append(r["rows"] + pos)
        pos += n
    assert st == state
    assert np.array_equal(np.concatenate(got), bits) and np.array_equal(np.concatenate(rows), rec["rows"])


@pytest.mark.parametrize("pllinc", [4096, 8192])
def test_power_of_two_increments_meet_both_equalities(pllinc):
    """The loop tests pll < 0x8000 at a transition and pll > 0xffff after the add; a kernel that reads a bit of the phase
    instead of comparing can be wrong only when the phase sits exactly on 0x8000 or 0x10000.  Floors: 100 and 100.
    Measured over the sixteen columns, as the slicer sees them: 521 transitions at 0x8000 and 2365 slices at 0x10000 at
    4096, 1729 and 6530 at 8192 (the eight columns of test_pll_with_a_sign_change_at_every_sample alone: 60 / 132 and
    426 / 2020)."""
    recs = [r for _, _, r in records(pllinc)]
    at_8000, at_10000 = sum(r["at_8000"] for r in recs), sum(r["at_10000"] for r in recs)
    print(pllinc, "transitions at 0x8000:", at_8000, "slices at 0x10000:", at_10000)
    assert at_8000 >= 100 and at_10000 >= 100


def drift(rec):
    whole = rec["blocks"][: TOTAL // pll_ref.BLK_TP]
    return whole[:, 1] - whole[:, 0]


@pytest.mark.parametrize("pllinc", [p for p in PLLINCS if p >= 256])
def test_fast_and_slow_drift_by_a_window_in_every_block(pllinc):
    """The time-parallel form tabulates a block on +-64 net nudges around the chunk's first value.  `fast` and `slow`
    move the net count by a whole window's width inside every 256-sample block, always the same way.  Floor: 120 from
    the start to the end of every whole block, on pll_ref.steered()'s signs from state 0 and on the slicer's decisions
    on the columns.  There the first block holds the table's delay, five samples without a sign change, each of which
    can cost it one nudge: floor 115 for that block, 120 for every other.

    Measured, fast / slow, least .. most per block: 256: 120..129 / 128..137; 1000: 120..126 / 124..140;
    3276: 121..128 / 127..136; 4096: 127..136 / 128..136; 8192: 128..133 / 131..133; 13107: 120..123 / 129..134;
    14000: 127..132 / 130..135; 14425: 123..128 / 127..132; 14426: 123..128 / 127..132 (first block as sliced: 117 at
    13107, 120 or more elsewhere).

    Plain greedy() gives 118..123 at 13107 `fast`: 9 of its 46 blocks are met at a phase that leaves only 118 or 119 of
    their samples below 0x8000.  steered() leaves sign changes out of the blocks before them (14 of 5 649 from state 0)
    and is greedy(), sign for sign, at every other increment and for `slow`."""
    for name, fast in (("fast", True), ("slow", False)):
        g, _ = pll_ref.steered(TOTAL, pllinc, fast)
        plain, _ = pll_ref.greedy(TOTAL, pllinc, fast)
        assert np.array_equal(g, plain) == (not (pllinc == 13107 and fast))
        from_zero = drift(pll_ref.pll_run(g, pllinc)[2]) * (1 if fast else -1)
        seen = drift(records(pllinc)[COLUMN_NAMES.index(name)][2]) * (1 if fast else -1)
        print(pllinc, name, "from state 0:", from_zero.min(), "..", from_zero.max(), " as sliced:", seen[0], "then", seen[1:].min(), "..", seen[1:].max())
        assert from_zero.min() >= 120 and seen[0] >= 115 and seen[1:].min() >= 120, name


@pytest.mark.parametrize("pllinc", [p for p in PLLINCS if p >= 16])
def test_edge_columns_stand_on_both_ends_of_the_window(pllinc):
    """pll_tp.hip's table holds the net counts centre - 64 .. centre + 62: centre + 64 is the first value past it, centre
    - 64 its lowest entry.  `edge_up` and `edge_down` move the count by exactly 64 in every block in which the phase
    allows it, then rest, so that pll_ref.walk() -- the kernel's walk, restated -- finds the count on exactly those two
    values at the end of a block, with blocks of the chunk still to go.  From 255 on every one of the 46 whole blocks
    offers its 64 nudges: a chunk per block upwards (floor 40 times on the value past the table; measured 46), a chunk
    per two blocks downwards (floor 20 times on the lowest entry; measured 23).  At 16 and 17 the phase rests below
    0x8000 for 2048 samples and above it for the next 2048, so half of the blocks move: floors 10 and 10 (measured
    24 / 11 and 22 / 12).  A kernel whose window reaches one candidate further than its table reads the next block's row
    there."""
    up = pll_ref.walk(records(pllinc)[COLUMN_NAMES.index("edge_up")][2]["blocks"])
    down = pll_ref.walk(records(pllinc)[COLUMN_NAMES.index("edge_down")][2]["blocks"])
    print(pllinc, "edge_up:", up, "edge_down:", down)
    assert up["past_table"] >= (40 if pllinc >= 255 else 10)
    assert down["lowest"] >= (20 if pllinc >= 255 else 10)
    if pllinc >= 255:
        assert set(drift(records(pllinc)[COLUMN_NAMES.index("edge_up")][2])) == {64}
        assert set(drift(records(pllinc)[COLUMN_NAMES.index("edge_down")][2])) == {-64}


def test_fast_fills_the_mask_and_the_pack_at_the_largest_increment():
    """pll_h3.hip keeps a 128-sample block's toggles in one 32-bit mask (at most 30 slices, bit 30) and the deframer a
    2048-sample segment's bits in 16 words.  Floors: 30 slices in some block, 460 bits in some segment.  Measured at
    14 426: 30 and 465 (`slow`: 28 and 437; the other columns: at most 29 and 454)."""
    for view in (records(14426)[FAST][2], pll_ref.pll_run(pll_ref.greedy(TOTAL, 14426, True)[0], 14426)[2]):
        print("most slices per 128:", view["per_128"].max(), "most bits per 2048:", view["per_2048"].max())
        assert view["per_128"].max() == 30 and 460 <= view["per_2048"].max() <= 16 * 32
    assert max(r["per_128"].max() for _, _, r in records(14426)) == 30       # and nothing goes past the design bound


def test_small_increments_leave_calls_and_segments_without_a_bit():
    """pllinc 1: 12 000 samples advance the phase by 12 000 of 65 536, no bit.  15 and 16: a bit every 4369 / 4096
    samples at rest, so most 2048-sample segments hold none (measured: 4 and 3 of 6 segments empty on `fast`, at least 3
    on every column)."""
    for bits, state, rec in records(1):
        assert bits.size == 0 and state[0] == TOTAL and rec["per_2048"].sum() == 0
    assert records(1)[0][2]["transitions"] > 10000
    for pllinc in (15, 16):
        for bits, _, rec in records(pllinc):
            assert bits.size >= 1
            assert 2 * np.count_nonzero(rec["per_2048"] == 0) >= rec["per_2048"].size
