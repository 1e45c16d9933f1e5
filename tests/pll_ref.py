"""The PLL stage, restated sample by sample, and the inputs its tests run (TEST INFRASTRUCTURE).

  pll_run()   the reference's loop (src/receiver.c:109-135) on one channel's slicer decisions, in Python integers:
              the NRZI-decoded bits, the carried (pll, prev, lastbit), and a record of what the input exercised --
              the equalities of the loop's two compares, the drift of the net nudge count per 256-sample block (the
              time-parallel kernel's window, pll_tp.hip), the slices per 128-sample block (the lane-per-channel kernel's
              32-bit mask, pll_h3.hip) and per 2048-sample segment (the deframer's pack).
  greedy()    the sign sequence with a transition at exactly the samples where the nudge is positive (`fast`: the phase
              runs ahead by one nudge at about every second sample) or negative (`slow`), made by running that loop.
  steered()   greedy(), with sign changes left out where that is what it takes to move the count by 120 in every block
              (`fast` at 13107); elsewhere the same signs.
  columns()   the int16 inputs of tests/test_pll_cpu.py and tests/test_pll_gpu.py, for a table that passes its input
              through (TAPS); signs_of() is what the slicer decides on them.
  walk()      the time-parallel kernel's walk through its chunks, restated on pll_run's record: how often an input
              puts the net count on the edges of the tabulated window.
  PLLINCS     the clock increments the suite runs: the ends of the range gnuais_batch_create() accepts (1, 14 426) and
              their neighbours, the threshold of the nudge (pllinc / 16 == 0 below 16) and of the time-parallel form,
              powers of two (every phase a multiple of the nudge: both compares meet their equalities), and the three
              values of the earlier tests.

The net nudge count c of the record is +1 for a transition met at pll < 0x8000 and -1 otherwise, counted from the call's
first sample, whatever the nudge's size (also 0)."""
import numpy as np

PLLINCS = (1, 15, 16, 17, 255, 256, 1000, 3276, 4096, 8192, 13107, 14000, 14425, 14426)

BLK_TP, BLK_H3, SEG = 256, 128, 2048

TAPS = np.zeros(9, dtype=np.float32)          # passes the input through, DELAY samples late
TAPS[4] = 1.0
DELAY = 5                                     # checked against the restatement's filter in tests/test_pll_cpu.py

HI, LO = 900, -900


def pll_run(signs, pllinc, state=None):
    """signs: 0 / 1 per sample (`out > 0`, receiver.c:111).  state = (pll, prev, lastbit), carried.
    Returns (bits uint8, state, record)."""
    pll, prev, lastbit = state if state is not None else (0, 0, 0)
    nudge = pllinc // 16
    bits, rows, cs = [], [], []
    c = n_trans = at_8000 = at_10000 = 0
    for i, curr in enumerate(np.asarray(signs).tolist()):
        if curr ^ prev:                                     # :113
            n_trans += 1
            if pll < 0x8000:                                # :114
                pll += nudge
                c += 1
            else:
                if pll == 0x8000:
                    at_8000 += 1
                pll -= nudge
                c -= 1
        prev = curr                                         # :120
        pll += pllinc                                       # :122
        if pll > 0xffff:                                    # :124
            if pll == 0x10000:
                at_10000 += 1
            bits.append(1 - (curr ^ lastbit))               # :128
            lastbit = curr
            pll &= 0xffff
            rows.append(i)
        cs.append(c)
    n = len(cs)
    rows = np.asarray(rows, dtype=np.int64)
    full = np.concatenate([[0], np.asarray(cs, dtype=np.int64)])     # c before sample i; full[n] = after the last
    blocks = np.zeros(((n + BLK_TP - 1) // BLK_TP, 4), dtype=np.int64)      # start, end, min, max
    for b in range(blocks.shape[0]):
        w = full[BLK_TP * b: min(BLK_TP * (b + 1), n) + 1]
        blocks[b] = (w[0], w[-1], w.min(), w.max())
    rec = {"transitions": n_trans, "at_8000": at_8000, "at_10000": at_10000, "blocks": blocks, "rows": rows,
           "per_128": np.bincount(rows // BLK_H3, minlength=(n + BLK_H3 - 1) // BLK_H3),
           "per_2048": np.bincount(rows // SEG, minlength=(n + SEG - 1) // SEG)}
    return np.asarray(bits, dtype=np.uint8), (pll, prev, lastbit), rec


SLOW, FAST, SILENT = 0, 1, 2


def greedy(total, pllinc, fast, state=None, per_block=None, first=0):
    """The signs (uint8 [total]) that change at exactly the samples where the loop's nudge is positive (`fast` true) or
    negative (false), from `state`.  `fast` may be an array of SLOW / FAST / SILENT per sample; SILENT holds the sign at
    0 (a transition where it was 1).  With `per_block` (one number, or one per block) the sign stops changing once the
    net nudge count has moved by that much inside the current 256-sample block; the blocks start at sample -first.
    Returns (signs, state)."""
    pll, prev, lastbit = state if state is not None else (0, 0, 0)
    nudge = pllinc // 16
    mode = np.broadcast_to(np.asarray(fast, dtype=np.int64), (total,)).tolist()
    out = []
    moved = 0
    caps = None if per_block is None else np.broadcast_to(per_block, ((total + first + BLK_TP - 1) // BLK_TP,)).tolist()
    for i, m in enumerate(mode):
        if (i + first) % BLK_TP == 0:
            moved = 0
        if m == SILENT:
            curr = 0
        elif caps is not None and moved >= caps[(i + first) // BLK_TP]:
            curr = prev
        else:
            curr = prev ^ 1 if (pll < 0x8000) == (m == FAST) else prev
        if curr ^ prev:
            pll += nudge if pll < 0x8000 else -nudge
            moved += 1
        prev = curr
        pll += pllinc
        if pll > 0xffff:
            lastbit = curr
            pll &= 0xffff
        out.append(curr)
    return np.asarray(out, dtype=np.uint8), (pll, prev, lastbit)


def _block(pll, pllinc, fast, cap, n):
    """greedy() over n samples with at most `cap` sign changes: (pll after them, sign changes made)"""
    nudge, c = pllinc // 16, 0
    for _ in range(n):
        if (pll < 0x8000) == fast and c < cap:
            pll += nudge if fast else -nudge
            c += 1
        pll = (pll + pllinc) & 0xffff
    return pll, c


def steered(total, pllinc, fast, state=None, floor=120, first=0):
    """greedy(), steered so that the net count moves by at least `floor` in EVERY whole 256-sample block (blocks start at
    sample -first; a first block shortened by `first` may fall short by as much).  Plain greedy() does that by itself
    at most increments, and then this IS greedy().  Where it does not -- at 13107 the phase arrives at 9 of 46 blocks so
    that only 118 or 119 of their samples lie below 0x8000 -- a block that could move further leaves its last sign
    changes out: every nudge left out holds the phase back by pllinc / 16, and the blocks behind it are met at a better
    phase.  The blocks' counts come from a depth-first search, the largest first; without a solution (or below 256,
    where no input moves the count that far in every block) the result is plain greedy()."""
    fast = bool(fast)
    pll = (state if state is not None else (0, 0, 0))[0]
    sizes = [BLK_TP - first] + [BLK_TP] * ((total + first) // BLK_TP - 1) if total + first >= BLK_TP else []
    plan, dead = [], set()

    def search(b, pll):
        if b == len(sizes):
            return True
        if (b, pll) in dead:
            return False
        most = _block(pll, pllinc, fast, total, sizes[b])[1]
        for cap in range(most, floor - (BLK_TP - sizes[b]) - 1, -1):
            plan.append(cap)
            if search(b + 1, _block(pll, pllinc, fast, cap, sizes[b])[0]):
                return True
            plan.pop()
        dead.add((b, pll))
        return False

    if pllinc < 256 or not search(0, pll):
        return greedy(total, pllinc, FAST if fast else SLOW, state)
    return greedy(total, pllinc, FAST if fast else SLOW, state, per_block=plan + [total], first=first)


def walk(blocks, chunk=32, half=64):
    """pll_tp.hip's walk over the blocks of one call, restated on pll_run's record: a chunk of at most `chunk` blocks
    tabulates every block's map on the net counts centre - half .. centre + half - 2 around the count at its first
    sample, and ends where the count, taken at a block's end, has left that window.  Returns how many chunks the call
    takes, how often the count stands on the first value PAST the table (centre + half) with blocks of the chunk still
    to go, and how often on the table's lowest value (centre - half)."""
    n, b0 = len(blocks), 0
    chunks = past = lowest = 0
    while b0 < n:
        b1, centre, i, v = min(b0 + chunk, n), int(blocks[b0][0]), 0, 0
        chunks += 1
        while i < b1 - b0:
            if not -half <= v <= half - 2:
                past += v == half
                break
            lowest += v == -half
            v = int(blocks[b0 + i][1]) - centre
            i += 1
        b0 += i
    return {"chunks": chunks, "past_table": int(past), "lowest": int(lowest)}


def idle(n, pllinc, state=None):
    """the state after n samples without a sign change"""
    pll, prev, lastbit = state if state is not None else (0, 0, 0)
    for _ in range(n):
        pll += pllinc
        if pll > 0xffff:
            lastbit = prev
            pll &= 0xffff
    return pll, prev, lastbit


def levels(signs, silent=None):
    x = np.where(np.asarray(signs) != 0, HI, LO)
    if silent is not None:
        x = np.where(silent, 0, x)
    return x.astype(np.int16)


def signs_of(x, history=None):
    """The slicer's decisions on x (int16 [len] or [len][n]) through TAPS: x > 0, DELAY samples late; `history` = the
    last DELAY samples of the calls before (zeros for a fresh batch)."""
    x = np.asarray(x)
    h = np.zeros((DELAY,) + x.shape[1:], dtype=x.dtype) if history is None else np.asarray(history)[-DELAY:]
    return (np.concatenate([h, x])[: x.shape[0]] > 0).astype(np.uint8)


COLUMN_NAMES = ("every_1", "every_2", "every_3", "every_7", "bursts", "alternating_rates", "coin", "mostly_every_1",
                "fast", "slow", "fast_slow_3000", "fast_bursts_700", "half_wave_8", "half_wave_16", "edge_up", "edge_down")


def columns(total, pllinc, rng=None):
    """int16 [total][16], COLUMN_NAMES.  The greedy columns are made for the state a fresh receiver has when its first
    sample arrives behind the table's delay, so that the slicer's decisions on them ARE greedy()'s signs.  pllinc 0 is
    the library's default, 0x10000 / 5."""
    pllinc = pllinc or 0x10000 // 5
    rng = rng if rng is not None else np.random.default_rng(123)
    t = np.arange(total)
    # the eight columns of test_hip_parity.py::test_pll_with_a_sign_change_at_every_sample
    cols = [np.where(t % 2, 900.0, -900.0),                                    # a transition at every sample
            np.where(t // 2 % 2, 900.0, -900.0), np.where(t // 3 % 2, 900.0, -900.0),
            np.where(t // 7 % 2, 900.0, -900.0),
            np.where((t // 700) % 2, np.where(t % 2, 900.0, -900.0), 0.0),     # bursts of them between silences
            np.where((t // 1500) % 2, np.where(t % 2, 900.0, -900.0), np.where(t // 5 % 2, 900.0, -900.0)),
            rng.choice([-500.0, 500.0], total),                                # a fair coin per sample
            np.where(rng.random(total) < 0.9, np.where(t % 2, 300.0, -300.0), 300.0)]
    start = idle(DELAY, pllinc)
    cols.append(levels(steered(total, pllinc, True, start, first=DELAY)[0]))
    cols.append(levels(steered(total, pllinc, False, start, first=DELAY)[0]))
    # the drift turns round every 3000 samples: inside a chunk of 32 blocks of the time-parallel form
    cols.append(levels(greedy(total, pllinc, np.where((t + DELAY) // 3000 % 2, SLOW, FAST), start)[0]))
    silent = ((t + DELAY) // 700) % 2 == 0
    cols.append(levels(greedy(total, pllinc, np.where(silent, SILENT, FAST), start)[0], silent))
    # exactly 8 and 16 samples per half wave: in step with pllinc 8192 and 4096
    cols.append(np.where(t // 8 % 2, 900.0, -900.0))
    cols.append(np.where(t // 16 % 2, 900.0, -900.0))
    # the net count moves by exactly 64 up / down in every 256-sample block the slicer's decisions fall into, then rests:
    # the first value past the time-parallel form's table, and the table's lowest value (walk())
    cols.append(levels(greedy(total, pllinc, FAST, start, per_block=64, first=DELAY)[0]))
    cols.append(levels(greedy(total, pllinc, SLOW, start, per_block=64, first=DELAY)[0]))
    x = np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1).astype(np.int16)
    assert x.shape[1] == len(COLUMN_NAMES)
    return x
