"""The signal records of the long frames and their share in the channel load, restated (TEST INFRASTRUCTURE; the binding
definition is in include/gnuais_hip.h under gnuais_batch_long_frame_signal).

Nothing is defined anew here.  A long record with time t and nbits gets frame_signal_ref's record -- the same q, S, j_lo,
nb, power, ferr and blocks, over the same block sums with the same v0 -- through
FrameSignalRef.records_for(long_records, long_records["t"]); the long records and their t come from long_ref.SampleRef (with
long_repair_ref's deframers where the repair is on); the channel load is occupancy_ref.OccupancyRef with the one number the
feature changes: LAG takes 1008 + 24 bits in place of 448 + 24 (LongOccupancyRef restates epochs() with it).

LongSignalRef is fed call by call like the device: run_iq() takes the I/Q of a call and the audio the stages in front of
the chain made of it, run_audio() an audio-type call, decode_bits() bits without samples."""
import numpy as np

import frame_signal_ref as fsr
import long_ref as lr
import long_repair_ref as lrr
import occupancy_ref as orf

B = 64
LONG_BITS = lr.LONG_MAX_BITS
SIGNAL_DTYPE = fsr.SIGNAL_DTYPE


def lag(pllinc: int = 0x10000 // 5, n_taps: int = 36, W: int = 0, max_bits: int = LONG_BITS) -> int:
    """LAG of the definition with the longest covering frame of max_bits bits (448: occupancy_ref.lag)"""
    return (max_bits + 24) * 65536 // pllinc + orf.pre_rows(pllinc) + (n_taps + 1) // 2 + W // 2 + B


class SampleRef(lr.SampleRef):
    """long_ref.SampleRef for any table, and with t = -1 for a frame that no segment of samples closed (decode_bits)"""

    def __init__(self, n_ch, taps=None, pllinc=0, repair=False):
        super().__init__(n_ch)
        if taps is not None or pllinc:
            from oracle_lib import Oracle
            self.o = Oracle(n_ch, taps, pllinc)
        if repair:
            self.ds = [lrr.RawLongDeframer() for _ in range(n_ch)]

    def t(self, c, f):
        try:
            return super().t(c, f)
        except AssertionError:
            return -1


class LongSignalRef:
    """short frames with times and records (frame_signal_ref.FrameSignalRef), long records with theirs"""

    def __init__(self, n_ch, taps=None, pllinc=0, afc_window=0, repair=False):
        self.n_ch, self.args = n_ch, (taps, pllinc, afc_window, repair)
        self.fs = fsr.FrameSignalRef(n_ch, taps, pllinc, afc_window)
        self.long = SampleRef(n_ch, taps, pllinc, repair)
        self.repair = repair
        self.lon = False
        self.lcalls = []                                    # (first row, v0 for the long frames this call closes)

    @property
    def n(self):
        return self.fs.ft.n

    def switch_on(self):
        """frame_signal, then long_frame_signal, at the current row"""
        self.fs.switch_on()
        self.long_switch_on()

    def long_switch_on(self):
        """long_frame_signal alone: a new run starts here; long records closed before it give (0, 0, 0).  (The short
        frames already queued keep their records on the device: drain them first.)"""
        self.lon = True
        self.fs.sums.reset(self.n)
        self.lcalls = []

    def long_switch_off(self):
        self.lon = False

    def reset(self):
        taps, pllinc, W, repair = self.args
        self.fs.reset()
        self.long = SampleRef(self.n_ch, taps, pllinc, repair)
        self.lcalls = []

    def run_iq(self, iq, audio):
        n0 = self.n
        self.fs.run_iq(iq, audio)
        self.long.run(audio)
        if self.lon:
            self.lcalls.append((n0, self.fs.sums.v0))

    def run_audio(self, audio):
        n0 = self.n
        self.fs.run_audio(audio)
        self.long.run(audio)
        if self.lon:
            self.lcalls.append((n0, self.n))               # v0 behind the call: its frames give (0, 0, 0)

    def decode_bits(self, bits_per_channel):
        self.fs.decode_bits(bits_per_channel)
        for d, p in zip(self.long.ds, bits_per_channel):
            d.feed(p)

    def long_records_for(self, rec):
        """frame_signal_ref's records of long records, by the calls since long_frame_signal was switched on"""
        saved, self.fs.calls = self.fs.calls, self.lcalls
        try:
            return self.fs.records_for(rec, rec["t"])
        finally:
            self.fs.calls = saved

    def drain_long(self):
        """(long records, their signal records) in the drain's order; consumes them"""
        if self.repair:
            rec = lrr.records_of(self.long.ds, self.long.t)[0]
        else:
            rec = lr.records(self.long.ds, self.long.t)
        for d in self.long.ds:
            d.closed = []
        return rec, self.long_records_for(rec)

    def drain(self):
        """the short frames: (frames, times, signal)"""
        return self.fs.drain()


class LongOccupancyRef(orf.OccupancyRef):
    """occupancy_ref.OccupancyRef with LAG of max_bits: epochs() restated with that one number; the long records are added
    with add_frames(records, records["t"]) like any frame"""

    def __init__(self, *a, max_bits=LONG_BITS, **k):
        super().__init__(*a, **k)
        self.max_bits = max_bits

    def epochs(self):
        starts = np.array([c[0] for c in self.calls], dtype=np.int64)
        per_run = {}
        for c, nbits, t in self.frames:
            k = int(np.searchsorted(starts, t, side="right")) - 1
            if k >= 0 and self.calls[k][1] >= 0:
                per_run.setdefault(self.calls[k][1], []).append((c, nbits, t))
        out = []
        L = lag(self.pllinc, self.n_taps, self.W, self.max_bits)
        for ri, r in enumerate(self.runs):
            b0 = -(-r["v0"] // B)
            n_final = 0
            while r["end"] > B * (b0 + (n_final + 1) * self.E) - 1 + L:
                n_final += 1
            if not n_final:
                continue
            j0, P = orf.block_power(np.concatenate(r["iq"]), r["v0"])
            assert j0 == b0
            codes = orf.code(P[:n_final * self.E])
            cover = np.zeros(codes.shape, dtype=bool)
            for c, nbits, t in per_run.get(ri, []):
                j_lo, nb = orf.cover_span(t, nbits, self.pllinc, self.n_taps, self.W, r["v0"])
                lo, hi = max(j_lo - b0, 0), min(j_lo + nb - b0, len(cover))
                if nb and hi > lo:
                    cover[lo:hi, c] = True
            before = np.zeros(self.n_ch, dtype=bool)
            for k in range(n_final):
                s = slice(k * self.E, (k + 1) * self.E)
                rec, words, before = orf.epoch_record(codes[s], cover[s], self.m, before)
                out.append((b0 + k * self.E, rec, words))
        return out


# ---- the base input LS9 -------------------------------------------------------------------------------------------------
LS9_ROWS = 6 * 8 * 1280
LS9_CALLS = (4096, 1, 2047, 5000)
_LS9 = {}


def ls9():
    """[61440][2][2] int16: gated long-payload bursts of seed 9 over noise, two channels"""
    if "x" not in _LS9:
        from gnuais_amd import synth
        _LS9["x"] = np.stack([synth.make_iq_stream(LS9_ROWS, seed=9, channel=c, sigma=800.0, amplitude=10000.0, gated=True,
                                                   payloads=lr.long_payloads())[0] for c in range(2)], axis=1)
    return _LS9["x"]


def ragged(total, pattern=LS9_CALLS):
    """[(first row, end row)] of calls of the pattern's lengths, repeated, over total rows"""
    out, a, i = [], 0, 0
    while a < total:
        e = min(a + pattern[i % len(pattern)], total)
        out.append((a, e))
        a, i = e, i + 1
    return out


def ls9_restated(pattern=LS9_CALLS):
    """LS9 through the restatements in ragged calls of the pattern (a frame's t depends on where its call began),
    computed once and left unchanged: dict(long, long_sig, short, short_t, short_sig)"""
    if pattern not in _LS9:
        import iq_ref
        x = ls9()
        ref = LongSignalRef(2)
        ref.switch_on()
        carry = None
        for a, e in ragged(LS9_ROWS, pattern):
            audio, carry = iq_ref.discriminate(x[a:e], carry)
            ref.run_iq(x[a:e], audio)
        rec, sig = ref.drain_long()
        fr, t, fsig = ref.drain()
        _LS9[pattern] = dict(long=rec, long_sig=sig, short=fr, short_t=t, short_sig=fsig)
    return _LS9[pattern]


def ls9_epochs(with_long: bool, E=64, margin=16, pattern=LS9_CALLS):
    """the final epochs of LS9 with occupancy switched on at row 0: with the long frames' cover and their LAG, or as the
    feature off gives them"""
    r = ls9_restated(pattern)
    occ = LongOccupancyRef(2, E, margin, max_bits=LONG_BITS if with_long else 448)
    for a, e in ragged(LS9_ROWS, pattern):
        occ.run_iq(a, ls9()[a:e])
    occ.add_frames(r["short"], r["short_t"])
    if with_long:
        occ.add_frames(r["long"], r["long"]["t"])
    return occ.epochs()
