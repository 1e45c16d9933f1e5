"""The signal power and carrier error of a frame, restated in NumPy int64 (TEST INFRASTRUCTURE; the binding definition
is in include/gnuais_hip.h under gnuais_batch_frame_signal).

  Rows.  n is the chain's row counter.  x[n] = (I, Q) is the int16 pair an I/Q-type call hands to the discriminator as
  row n.  v0 is the first row of the current unbroken run of I/Q-type calls: set to the current n when the feature is
  switched on, at a reset, and when the first I/Q-type call follows an audio-type run call (while an audio-type call
  runs, v0 counts as the row behind it).  The previous pair of x[v0] is (0, 0): the stage's own carry.
  Per row, exact integers:  P = I^2 + Q^2,  r = I Ip + Q Qp,  i = Q Ip - I Qp.
  Per block.  Block j covers rows [64 j, 64 j + 64); P_j, R_j, I_j are the int64 sums over it (rows before v0: zero).
  Per frame with time t and nbits, d_f = (n_taps + 1) // 2, W the AFC window:
      q = t - d_f - W/2,  S = floor((nbits + 24) 65536 / pllinc),  j_lo = ceil((q - S) / 64),  j_hi = floor((q + 1) / 64),
      nb = j_hi - j_lo.   (0, 0, 0) when t < 0, nb <= 0 or 64 j_lo < v0.  Otherwise
      power = floor(sum P_j / (64 nb)),  ferr = afc_ref.estimate(sum R_j, sum I_j),  blocks = nb.

FrameSignalRef carries the block sums and tests/frame_time_ref.py's FrameTimeRef, fed call by call like the device."""
import numpy as np

import afc_ref
import frame_time_ref as ftr

B = 64
SIGNAL_DTYPE = np.dtype([("power", "<u4"), ("ferr", "<i2"), ("blocks", "<u2")])


def span(t: int, nbits: int, pllinc: int, n_taps: int = 36, W: int = 0, v0: int = 0):
    """(j_lo, nb) of the definition, (0, 0) where the record is (0, 0, 0); Python's // is floor for negative values"""
    if t < 0:
        return 0, 0
    q = t - (n_taps + 1) // 2 - W // 2
    S = ((nbits + 24) * 65536) // pllinc
    j_lo = -((S - q) // B)                                  # ceil((q - S) / 64)
    nb = (q + 1) // B - j_lo
    if nb <= 0 or B * j_lo < v0:
        return 0, 0
    return j_lo, nb


def row_terms(iq, prev):
    """P, r, i as exact int64 of pairs iq [len][N][2] after prev [N][2]"""
    iq = np.asarray(iq, dtype=np.int16)
    before = np.concatenate([np.asarray(prev, dtype=np.int16)[None], iq[:-1]], axis=0)
    I, Q = iq[..., 0].astype(np.int64), iq[..., 1].astype(np.int64)
    r, i = afc_ref.products(iq, before)
    return I * I + Q * Q, r, i


def record(sums, nb: int):
    """one record from the sums (P, R, I) over nb blocks"""
    out = np.zeros((), dtype=SIGNAL_DTYPE)
    if nb > 0:
        out["power"] = int(sums[0]) // (B * nb)
        out["ferr"] = afc_ref.estimate(np.int64(sums[1]), np.int64(sums[2]))
        out["blocks"] = nb
    return out


class BlockSums:
    """The block sums of n_ch channels: [block][n_ch][3] int64 from block `base` on (0 unless the clocks start at a
    large row: blk[k] is block base + k), fed call by call."""

    def __init__(self, n_ch: int, base: int = 0):
        self.n_ch, self.base = n_ch, int(base)
        self.reset(self.base * B)

    def reset(self, n: int):
        """a new run of I/Q-type calls starts at row n"""
        self.v0 = self.end = n
        self.carry = np.zeros((self.n_ch, 2), dtype=np.int16)
        if not hasattr(self, "blk"):
            self.blk = np.zeros((0, self.n_ch, 3), dtype=np.int64)

    def feed(self, n0: int, iq):
        """rows [n0, n0 + len) of an I/Q-type call"""
        iq = np.asarray(iq, dtype=np.int16)
        if n0 != self.end:
            self.reset(n0)                                  # an audio-type call came between
        if n0 == self.v0:
            self.blk = self.blk[:n0 // B - self.base]       # the rows of block v0 div 64 before v0 count as zero
        P, r, i = row_terms(iq, self.carry)
        n1 = n0 + iq.shape[0]
        need = -(-n1 // B) - self.base
        if need > self.blk.shape[0]:
            self.blk = np.concatenate([self.blk, np.zeros((need - self.blk.shape[0], self.n_ch, 3), dtype=np.int64)])
        np.add.at(self.blk, np.arange(n0, n1) // B - self.base, np.stack([P, r, i], axis=-1))
        self.carry = iq[-1].copy()
        self.end = n1

    def blocks(self, j0: int, count: int) -> np.ndarray:
        assert j0 >= self.base
        return self.blk[j0 - self.base:j0 - self.base + count].copy()


class FrameSignalRef:
    """frames, times and signal records of n_ch channels; run_iq() takes the I/Q of a call and the audio the stages in
    front of the chain made of it (iq_ref / afc_ref), run_audio() an audio-type call"""

    def __init__(self, n_ch: int, taps=None, pllinc: int = 0, afc_window: int = 0, rows: int = 0, bits=None):
        """rows, bits: where the clocks start (gnuais_batch_set_clock)"""
        self.ft = ftr.FrameTimeRef(n_ch, taps, pllinc, rows, bits)
        self.n_ch, self.W = n_ch, afc_window
        self.n_taps = 36 if taps is None else len(taps)
        self.pllinc = pllinc or 0x10000 // 5
        self.sums = BlockSums(n_ch, rows // B)
        self.on = False
        self.calls = []                                     # (first row, v0 for the frames this call closes)

    def switch_on(self):
        self.on = True
        self.sums.reset(self.ft.n)
        self.calls = []                                     # frames of earlier calls: (0, 0, 0)

    def reset(self, rows: int = 0, bits=None):
        """a reset, then set_clock(rows, bits)"""
        self.ft.reset(rows, bits)
        if rows // B != self.sums.base:
            self.sums = BlockSums(self.n_ch, rows // B)
        self.sums.reset(rows)
        self.calls = []

    def run_iq(self, iq, audio):
        n0 = self.ft.n
        if self.on:
            self.sums.feed(n0, iq)
            self.calls.append((n0, self.sums.v0))
        self.ft.run(audio)

    def run_audio(self, audio):
        n0 = self.ft.n
        self.ft.run(audio)
        if self.on:
            self.calls.append((n0, self.ft.n))              # v0 behind the call: its frames give (0, 0, 0)

    def decode_bits(self, bits_per_channel):
        self.ft.decode_bits(bits_per_channel)

    def records_for(self, fr, t) -> np.ndarray:
        """the records of frames fr with times t (any frames of the calls since the switch / the reset)"""
        sig = np.zeros(len(fr), dtype=SIGNAL_DTYPE)
        starts = np.array([c[0] for c in self.calls], dtype=np.int64)
        for k in range(len(fr)):
            if t[k] < 0 or not len(starts):
                continue
            c = int(np.searchsorted(starts, t[k], side="right")) - 1
            if c < 0:
                continue                                    # closed before the feature was switched on
            j_lo, nb = span(int(t[k]), int(fr["nbits"][k]), self.pllinc, self.n_taps, self.W, self.calls[c][1])
            if nb:
                sig[k] = record(self.sums.blocks(j_lo, nb)[:, int(fr["channel"][k])].sum(axis=0), nb)
        return sig

    def drain(self):
        """(frames, times, signal) in the drain's order"""
        fr, t = self.ft.drain()
        return fr, t, self.records_for(fr, t)
