"""One input and its expectations for the tests that queue calls without waiting (tests/test_tail_pipelined_gpu.py), and
the conditions that make that input worth running (tests/test_tail_cases_cpu.py).  TEST INFRASTRUCTURE, no GPU.

Nothing here restates a stage: build() only feeds the existing restatements the same calls the device gets --
iq_ref.discriminate for the audio, long_ref.SampleRef for the oracle's slices per segment and the definition's t,
repair_ref / long_repair_ref bit by bit for the frames and their repairs, frame_signal_ref for the records,
occupancy_ref for the epochs -- and puts their results in the order the drains deliver.

The input: 70 channels (one full wave of D' and a ragged one) of 48 slots of gated GMSK bursts.  Channel c carries a
long burst of long_ref.long_payloads() every seven slots from slot 3 c mod 7 on, the sizes turned by c, and position
reports in four of five of the slots between; its noise is one of four levels, so that some short and some long frames
fail the CRC by one symbol.  No channel is a turned copy of another: bursts start in other slots, carry other reports
and other noise, so no two calls leave equal hand-off sets behind.  For the duplicate merges, channels c and c + 35
carry the same report wherever both carry one (their long bursts and their noise differ), and a long burst's bytes
follow from its size alone, so channels whose long bursts of one size start in the same slot hear one transmission.

The bits of a channel do not depend on how the rows are cut into calls; only the times, and what follows from them, do.
The bit-by-bit part is therefore computed once per (first row, row of a protodec_reset) and shared by the call plans."""
import functools
from types import SimpleNamespace

import numpy as np

import frame_signal_ref as fsr
import iq_ref
import long_ref as lr
import long_repair_ref as lrr
import occupancy_ref as orf
import repair_ref as rr
from gnuais_amd import synth

N_CH = 70
TOTAL = 6 * 8 * 1280
RAGGED = (4096, 1, 2047, 5000, 33, 7000)
MAX_LEN = max(RAGGED)
E, MARGIN = 64, 16                      # occupancy: epochs of 4096 rows, 14 final in TOTAL rows
AMPLITUDE, SIGMAS = 3000.0, (250.0, 400.0, 550.0, 700.0)
EVERY, LONG_SLOTS = 7, 5                # a long burst every seven slots; the longest takes five
TWINS = 35                              # channels c and c + 35 hear the same position reports, where both hear one
UNIQUE_W = 64                           # the window of both duplicate merges, in rows


def plan(name):
    """the lengths of the calls: "ragged" (the pattern RAGGED over and over, 22 calls) or "equal" (48 calls of 1280)"""
    if name == "equal":
        return [1280] * (TOTAL // 1280)
    out = []
    while sum(out) < TOTAL:
        out.append(min(RAGGED[len(out) % len(RAGGED)], TOTAL - sum(out)))
    return out


def payloads_of(c):
    """make_iq_stream's `payloads` for channel c"""
    first = 3 * c % EVERY
    sizes = tuple(np.roll(lr.LONG_BYTES[:6], -c))
    pick = lr.long_payloads(sizes, EVERY)

    def payloads(rng, slot):
        if slot >= first and (slot - first) % EVERY < LONG_SLOTS:
            return pick(rng, slot - first)
        report = synth.random_position_report(np.random.default_rng([31, slot, c % TWINS]))
        return report if rng.random() < 0.8 else None
    return payloads


@functools.lru_cache(maxsize=None)
def iq_input():
    """int16 [TOTAL][N_CH][2]"""
    x = np.stack([synth.make_iq_stream(TOTAL, seed=31, channel=c, amplitude=AMPLITUDE, sigma=SIGMAS[c % len(SIGMAS)],
                                       payloads=payloads_of(c), gated=True)[0] for c in range(N_CH)], axis=1)
    x.setflags(write=False)
    return x


class Collector:
    """what SampleRef feeds: keeps the bits (the deframers get them in decode(), once for every plan)"""

    def __init__(self):
        self.fed, self.parts = 0, []

    def feed(self, bits):
        self.parts.append(np.asarray(bits, dtype=np.uint8))
        self.fed += len(bits)


_DECODED = {}


def decode(key, streams, cuts):
    """the bit-by-bit restatements over each channel's bits, a protodec_reset() in front of bit cuts[c] (None: none):
    the chain's frames with the repairs, D''s with theirs, and the counters of both"""
    if key in _DECODED:
        return _DECODED[key]
    short, long_ = [rr.Deframer() for _ in streams], [lrr.RawLongDeframer() for _ in streams]
    for c, bits in enumerate(streams):
        parts = [bits] if cuts is None else [bits[:cuts[c]], bits[cuts[c]:]]
        for i, part in enumerate(parts):
            if i:
                short[c].protodec_reset()
                long_[c].protodec_reset()
            short[c].feed(part)
            long_[c].feed(part)
    frames, repaired, counters = rr.records_of(short)
    records, counters3 = lrr.records_of(long_)              # t = -1: build() fills in the plan's
    spans = {}                                              # (channel, stamp) -> raw bits of the frame behind the record
    for c, d in enumerate(long_):
        for f in d.closed:
            spans[c, f["end_bit"]] = len(f["raw"])
    out = SimpleNamespace(frames=frames, repaired=repaired, counters=counters, long_records=records,
                          long_counters3=counters3, long_fsm=[d.fields() for d in long_], long_spans=spans)
    _DECODED[key] = out
    return out


@functools.lru_cache(maxsize=None)
def build(plan_name, first_call=0, protodec_at=None):
    """The expectations of the calls plan(plan_name)[first_call:] on a batch fresh from create or reset(), with a
    protodec_reset() in front of call protodec_at (None: none).  -> a namespace:
      calls            [(lo, hi)]: the rows of iq_input() each call takes
      frames, times, signal      drain_frames_signal()
      repaired, counters         repaired(), counters() as [n][3]
      long_records, long_counters3, long_fsm     drain_long_frames(), (delivered, failed, repaired), long_fsm_state()
      occ_first, occ_records     drain_occupancy()
      worth            what tests/test_tail_cases_cpu.py asserts of the input"""
    from oracle_lib import FRAME_DTYPE
    lens = plan(plan_name)
    edges = np.cumsum([0] + lens)
    calls = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])][first_call:]
    row0 = calls[0][0]
    x = iq_input()
    sample = lr.SampleRef(N_CH)
    sample.ds = [Collector() for _ in range(N_CH)]
    sig = fsr.FrameSignalRef(N_CH)
    sig.switch_on()
    occ = orf.OccupancyRef(N_CH, E, MARGIN)
    carry, cuts, ends, final_after = None, None, [], []
    for i, (lo, hi) in enumerate(calls):
        if protodec_at is not None and first_call + i == protodec_at:
            cuts = [d.fed for d in sample.ds]
            sig.ft.protodec_reset()
        audio, carry = iq_ref.discriminate(x[lo:hi], carry)
        occ.run_iq(lo - row0, x[lo:hi])
        sig.run_iq(x[lo:hi], audio)
        sample.run(audio)
        ends.append([d.fed for d in sample.ds])
        final_after.append(sum(1 for k in range(TOTAL // (64 * E) + 1) if hi - row0 > 64 * (k + 1) * E - 1 + orf.lag(sig.pllinc)))
    streams = [np.concatenate(d.parts) for d in sample.ds]
    dec = decode((row0, None if cuts is None else calls[protodec_at - first_call][0]), streams, cuts)

    frames = np.zeros(len(dec.frames), dtype=FRAME_DTYPE)
    for i, r in enumerate(dec.frames):
        frames[i] = r
    stamp = lambda r: int(r["end_bit"]) | ((int(r["flags"]) >> 1 & 31) << 32)
    times = np.array([sample.t(int(r["channel"]), {"index": stamp(r)}) for r in frames], dtype=np.int64)
    signal = sig.records_for(frames, times)
    # the oracle's own frames, times and records are the part that was not repaired
    wf, wt, ws = sig.drain()
    rep = (frames["flags"] & rr.FRAME_REPAIRED) != 0
    assert frames[~rep].tobytes() == wf.tobytes() and np.array_equal(times[~rep], wt) and signal[~rep].tobytes() == ws.tobytes()

    long_records = dec.long_records.copy()
    for i in range(len(long_records)):
        long_records["t"][i] = sample.t(int(long_records["channel"][i]), {"index": stamp(long_records[i])})
    occ.add_frames(frames, times)
    epochs = occ.epochs()

    ends = np.array(ends, dtype=np.int64)                   # [call][channel]: bits fed when the call ends
    across = 0
    for r in long_records:
        c, e = int(r["channel"]), stamp(r)
        across += bool(np.any((ends[:-1, c] > e - dec.long_spans[c, e]) & (ends[:-1, c] <= e)))
    worth = dict(long_channels=len(set(long_records["channel"].tolist())), long_across_calls=across,
                 long_repaired=int(dec.long_counters3[:, 2].sum()), short_repaired=int(dec.repaired.sum()),
                 long_received=int(dec.long_counters3[:, 0].sum()), short_received=int(dec.counters[:, 0].sum()),
                 epochs=len(epochs), epochs_before_the_last_call=final_after[-2], calls=len(calls))
    return SimpleNamespace(calls=calls, frames=frames, times=times, signal=signal, repaired=dec.repaired,
                           counters=dec.counters, long_records=long_records, long_counters3=dec.long_counters3,
                           long_fsm=dec.long_fsm, occ_first=[e[0] for e in epochs], occ_records=[e[1] for e in epochs],
                           worth=worth)


def heard(e, rows):
    """what the heard drains deliver for the expectations e at chain row `rows`: (drain_frames_heard(),
    drain_long_frames_heard()), from heard_ref and long_unique_ref"""
    import heard_ref as hr
    import long_unique_ref as lur
    return (hr.HeardRef(UNIQUE_W).push_heard(e.frames, e.times, rows, e.signal),
            lur.LongUniqueRef(UNIQUE_W).push_heard(e.long_records, rows))
