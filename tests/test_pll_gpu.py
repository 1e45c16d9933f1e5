"""The PLL stage (pll_h3.hip, pll_tp.hip) over every clock increment gnuais_batch_create() accepts, against the plain
per-sample loop of tests/pll_ref.py.

Every case compares, on every channel and after every call,
  * last_bits() and pll_state() with pll_ref.pll_run on the device's OWN last_signs() of that call, the carried state
    taken from the reference and never from the device: the FIR is out of the comparison;
  * bits, frames, counters, PLL carry and deframer state with the CPU restatement (chain_parity.run_both);
  * gnuais_batch_info("pll_form"), the form the launch took, with the limits restated here from the comment above
    pll_tp_applicable() (pll_tp.hip).  If those limits are moved on purpose, tp_applies() moves with them.
What the inputs exercise (equalities of both compares, a window's drift per block, both ends of the time-parallel form's
table, 30 slices in a block, 465 bits in a segment, calls without a bit) is asserted on the CPU in tests/test_pll_cpu.py."""
import functools

import numpy as np
import pytest

import pll_ref
from chain_parity import fsm_rows, run_both
from gnuais_amd import synth
from pll_ref import COLUMN_NAMES, PLLINCS

pytestmark = pytest.mark.gpu

TOTAL = 12000
RAGGED = [4097, 255, 1, 2048, 256, 257, 3086]


def tp_applies(n, pllinc):
    """pll_tp.hip, above pll_tp_applicable(): a call long enough to be worth it (one block of 256), at most 1024 blocks,
    the unwrapped phase 65536 + n * (pllinc + pllinc / 16) below 2^31, a nudge that is not 0"""
    return n >= 256 and (n + 255) // 256 <= 1024 and 65536 + n * (pllinc + pllinc // 16) < 2 ** 31 and pllinc >= 16


@functools.lru_cache(maxsize=None)
def columns(total, pllinc):
    x = pll_ref.columns(total, pllinc)
    return x


class EachCall:
    """run_both()'s hook: the device's bits and carry of every call == pll_run on its own signs of that call"""

    def __init__(self, n_ch, pllinc, variant, taps_pass_through=True):
        self.state = [None] * n_ch
        self.pllinc, self.variant, self.pass_through = pllinc or 0x10000 // 5, variant, taps_pass_through
        self.history = None
        self.forms, self.counts, self.fsm, self.records = [], [], [], []

    def __call__(self, b, o, i, seg, bits):
        n, n_ch = seg.shape
        signs = b.last_signs(n)
        if self.pass_through:           # and they are the signs tests/test_pll_cpu.py measured
            assert np.array_equal(signs.T, pll_ref.signs_of(seg, self.history)), i
            self.history = np.concatenate([np.zeros_like(seg[:pll_ref.DELAY]) if self.history is None else self.history, seg])[-pll_ref.DELAY:]
        p = b.pll_state()
        recs = []
        for c in range(n_ch):
            want, self.state[c], rec = pll_ref.pll_run(signs[c], self.pllinc, self.state[c])
            assert np.array_equal(bits[c], want), (i, c, len(bits[c]), len(want))
            assert (int(p["pll"][c]), int(p["prev"][c]), int(p["lastbit"][c])) == self.state[c], (i, c)
            recs.append(rec)
        form = b.info("pll_form")
        assert form == (7 if self.variant == 7 and tp_applies(n, self.pllinc) else 8), (i, n, form)
        self.forms.append(int(form))
        self.counts.append([len(v) for v in bits])
        self.fsm.append(fsm_rows(b))
        self.records.append(recs)


def run(x, chunks, pllinc, variant, taps=pll_ref.TAPS):
    x = x[: sum(chunks)]
    hook = EachCall(x.shape[1], pllinc, variant, taps is pll_ref.TAPS)
    o, b = run_both(x, list(chunks), x.shape[1], taps=taps, pllinc=pllinc, pll_variant=variant, each_call=hook)
    return o, b, hook


# ---------------------------------------------------------------- every increment, both forms

@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("pllinc", PLLINCS)
def test_every_increment_both_forms(pllinc, variant):
    """The sixteen columns of pll_ref.columns(): one call of 12 000 samples, then ragged calls on a fresh batch.  With
    pll_variant 7 the time-parallel form runs every call of at least 256 samples at every pllinc >= 16, and the
    lane-per-channel form the calls of 255 and 1 sample and every call at 1 and 15; with 8 it is always that one."""
    x = columns(TOTAL, pllinc)
    _, b, hook = run(x, [TOTAL], pllinc, variant)
    assert hook.forms == [7 if variant == 7 and pllinc >= 16 else 8]
    b.close()
    _, b, hook = run(x, RAGGED, pllinc, variant)
    assert hook.forms == [7 if variant == 7 and pllinc >= 16 and n >= 256 else 8 for n in RAGGED]
    b.close()


def test_pll_form_is_zero_before_any_call_and_after_a_reset():
    from chain_parity import batch, dev
    b = batch(2, taps=pll_ref.TAPS, pllinc=4096, max_len=512)
    assert b.info("pll_form") == 0
    b.run(dev(columns(512, 4096)[:, :2]))
    assert b.info("pll_form") == 7                  # two channels: the time-parallel form by itself (pll_variant 0)
    b.run(dev(columns(512, 4096)[:255, :2]))
    assert b.info("pll_form") == 8
    b.reset()
    assert b.info("pll_form") == 0


# ---------------------------------------------------------------- channel counts, lane per channel

@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("pllinc", [4096, 8192, 14426])
def test_channel_counts_on_the_lane_per_channel_form(pllinc, n_ch):
    """One live lane, a wave one short of full, a full wave, a second wave with one lane, three waves: the columns
    repeated with a time shift per channel, so that neighbouring lanes differ in everything -- `every_1` has 16 times
    the transitions of `half_wave_16`, and a wave's rows are as many as its busiest lane's."""
    base = columns(TOTAL, pllinc)
    k = np.arange(n_ch)
    pick = (k + COLUMN_NAMES.index("fast")) % base.shape[1] if n_ch == 1 else k % base.shape[1]     # the single channel: `fast`
    x = np.stack([np.roll(base[:, j], 37 * (c // base.shape[1])) for c, j in enumerate(pick)], axis=1)
    _, b, hook = run(x, RAGGED + [TOTAL - sum(RAGGED)], pllinc, 8)
    assert set(hook.forms) == {8}
    b.close()


# ---------------------------------------------------------------- messages at other rates

@functools.lru_cache(maxsize=None)
def stream(sps):
    total = 30 * 256 * sps
    x = np.stack([synth.make_stream(total, seed=31, channel=c, sps=sps, sigma=1000)[0] for c in range(6)], axis=1)
    return x


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("table", ["pass_through", "reference"])
@pytest.mark.parametrize("sps", [8, 16])
def test_messages_at_eight_and_sixteen_samples_per_bit(sps, table, variant):
    """Thirty slots of messages on six channels at pllinc 8192 and 4096, through the table that passes the input on and
    through the reference's own: the deframer and the CRC stage are fed behind the new increments.  The restatement
    decodes 95 / 93 frames at 8 samples per bit and 91 / 95 at 16; floor: 85 in each of the four runs."""
    x = stream(sps)
    taps = pll_ref.TAPS if table == "pass_through" else None
    o, b, _ = run(x, [x.shape[0]], 0x10000 // sps, variant, taps=taps)
    print(sps, table, "frames:", len(o.frames()))
    assert len(o.frames()) >= 85
    b.close()
    o2, b, hook = run(x, RAGGED + [x.shape[0] - sum(RAGGED)], 0x10000 // sps, variant, taps=taps)
    assert o2.frames().tobytes() == o.frames().tobytes()
    assert hook.forms[-1] == variant
    b.close()


# ---------------------------------------------------------------- the limits of the time-parallel form

def at_the_limit(pllinc, length):
    """`fast` and `slow` on two channels: a first call that leaves `fast`'s phase as near 0xffff as any length from 256 to
    700 samples does (the state the long call starts from is then at the top of its range), then calls of `length` and,
    on a fresh batch, of `length + 1` samples.  The time-parallel form takes the first and must refuse the second."""
    assert tp_applies(length, pllinc) and not tp_applies(length + 1, pllinc)
    start = pll_ref.idle(pll_ref.DELAY, pllinc)
    x = np.stack([pll_ref.levels(pll_ref.greedy(700 + length + 1, pllinc, fast, start)[0]) for fast in (1, 0)], axis=1)
    s = pll_ref.signs_of(x[:700])[:, 0]
    _, st, _ = pll_ref.pll_run(s[:256], pllinc)
    best, n0 = st[0], 256
    for n in range(257, 701):
        _, st, _ = pll_ref.pll_run(s[n - 1:n], pllinc, st)
        if st[0] > best:
            best, n0 = st[0], n
    assert best > 0xffff - pllinc
    for n, form in ((length, 7), (length + 1, 8)):
        _, b, hook = run(x, [n0, n], pllinc, 7)
        assert hook.forms == [7, form]
        assert max(r["transitions"] for r in hook.records[1]) > n // 3
        b.close()


def test_phase_limit_of_the_time_parallel_form():
    """14 426: the longest call whose unwrapped phase 65536 + L * (pllinc + pllinc / 16) stays below 2^31 (140 106 samples), and one more"""
    length = (2 ** 31 - 65536 - 1) // (14426 + 14426 // 16)
    at_the_limit(14426, length)


def test_block_count_limit_of_the_time_parallel_form():
    """4096: 1024 blocks of 256 samples, and one sample more"""
    at_the_limit(4096, 262144)


# ---------------------------------------------------------------- calls without bits

def untouched(hook, i):
    """channels that got no bit in call i have the deframer state they had before it"""
    for c, n in enumerate(hook.counts[i]):
        if n == 0 and i > 0:
            assert hook.fsm[i][c] == hook.fsm[i - 1][c], (i, c)


@pytest.mark.parametrize("variant", [7, 8])
def test_one_bit_in_seventy_thousand_samples(variant):
    """pllinc 1: the phase needs 65 536 samples for one bit.  A call of 70 000 samples holds exactly one, the calls of 1
    and 2048 samples behind it none (no segment of theirs has one: last_bits() is empty, the deframer's state is what it
    was), the call of 65 536 the second.  pllinc / 16 == 0: no nudge, and the lane-per-channel form whatever is asked."""
    chunks = [70000, 1, 2048, 65536]
    x = columns(sum(chunks), 1)[:, [COLUMN_NAMES.index(n) for n in ("every_1", "coin", "fast", "half_wave_16")]]
    _, b, hook = run(x, chunks, 1, variant)
    assert hook.counts == [[1] * 4, [0] * 4, [0] * 4, [1] * 4] and set(hook.forms) == {8}
    for i in (1, 2):
        untouched(hook, i)
    b.close()


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("pllinc", [15, 255])
def test_ragged_calls_mostly_without_bits(pllinc, variant):
    """15 (no nudge, a bit every 4369 samples) and 255 (a bit every 257 at rest, every 242 at the most): calls around the
    128-, 256- and 2048-sample edges of the two kernels' blocks and of the segments.  At 15 the 11 694 samples hold at
    most 3 bits per channel, so at least 10 of the 13 calls bring a channel none; at 255 the calls of 127, 128 and 129
    samples hold at most 2 between them, so at least one of them brings none."""
    chunks = [127, 128, 129, 255, 256, 257, 1, 2047, 2048, 2049, 1, 4096, 300]
    _, b, hook = run(columns(sum(chunks), pllinc), chunks, pllinc, variant)
    empty = sum(1 for i in range(len(chunks)) for n in hook.counts[i] if n == 0)
    print(pllinc, "calls x channels without a bit:", empty, "of", len(chunks) * len(COLUMN_NAMES))
    assert empty >= (10 if pllinc == 15 else 1) * len(COLUMN_NAMES)
    for i in range(len(chunks)):
        untouched(hook, i)
    b.close()
