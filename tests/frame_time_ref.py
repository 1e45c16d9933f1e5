"""The receive time of a frame, restated (TEST INFRASTRUCTURE; the definition is in include/gnuais_hip.h under
gnuais_batch_frame_times).

  n counts the rows the chain has taken since create / reset.  A call that takes rows [n0, n0 + len) is cut into
  segments of 2048 rows; segment s has l_s rows, c_s of which slice.  The bit with index e that closed a frame is the
  j-th slice of some segment s of the call that fed it:   t(e) = n0 + 2048 s + floor((2 j + 1) l_s / (2 c_s)).
  Bits fed without samples (decode_bits) give -1.

FrameTimeRef gets c_s from the CPU oracle by feeding it one segment at a time (its state carries across calls, so the
frames are those of the whole call) and applies the formula to the oracle's frames.  pll_rows() is a per-sample
transcription of the reference's loop (src/receiver.c:109-135) that gives the true slicing row of every bit, for the
accuracy test; time_map() restates gnuais_batch_time_map()."""
import numpy as np

from oracle_lib import Oracle

SEG = 2048


def interp(n0: int, s: int, j: int, l_s: int, c_s: int) -> int:
    return n0 + SEG * s + ((2 * j + 1) * l_s) // (2 * c_s)


def stamp(frames: np.ndarray) -> np.ndarray:
    """the 37-bit index of the bit that closed each frame: end_bit and flags[5:1]"""
    return frames["end_bit"].astype(np.int64) | (((frames["flags"].astype(np.int64) >> 1) & 31) << 32)


class FrameTimeRef:
    def __init__(self, n_ch: int, taps=None, pllinc: int = 0):
        self.o = Oracle(n_ch, taps, pllinc)
        self.n_ch = n_ch
        self.reset()

    def reset(self):
        self.o.reset()
        self.o.clear_frames()
        self.n = 0                                          # rows taken
        self.fed = np.zeros(self.n_ch, dtype=np.int64)      # bits fed per channel
        # one entry per segment fed: (first row or -1, rows, bits fed before it per channel, bits in it per channel)
        self.segs = []

    def protodec_reset(self):
        self.o.protodec_reset()                             # the bit count and n stay

    def run(self, x: np.ndarray):
        """one call: x int16 [len][n_ch]"""
        x = np.ascontiguousarray(x, dtype=np.int16)
        for s0 in range(0, x.shape[0], SEG):
            seg = x[s0:s0 + SEG]
            bits = self.o.run(seg, want_bits=True)["bits"]
            cnt = np.array([len(b) for b in bits], dtype=np.int64)
            self.segs.append((self.n + s0, seg.shape[0], self.fed.copy(), cnt))
            self.fed += cnt
        self.n += x.shape[0]

    def decode_bits(self, bits_per_channel):
        cnt = np.array([len(b) for b in bits_per_channel], dtype=np.int64)
        for c, b in enumerate(bits_per_channel):
            if len(b):
                self.o.decode_bits(c, np.asarray(b, dtype=np.uint8))
        self.segs.append((-1, 0, self.fed.copy(), cnt))
        self.fed += cnt

    def drain(self):
        """(frames in the drain's order, int64 times); consumes the oracle's frames"""
        fr = self.o.frames()
        self.o.clear_frames()
        times = np.full(len(fr), -2, dtype=np.int64)
        if len(fr):
            base = np.stack([s[2] for s in self.segs])      # [segments][n_ch]
            e = stamp(fr)
            for i, (c, ei) in enumerate(zip(fr["channel"], e)):
                # the last segment that starts at or before the bit (one without bits shares its start with the next)
                k = int(np.searchsorted(base[:, c], ei, side="right")) - 1
                row0, l_s, b0, cnt = self.segs[k]
                j = int(ei - b0[c])
                assert 0 <= j < cnt[c], (i, c, ei, k)
                times[i] = -1 if row0 < 0 else interp(row0, 0, j, l_s, int(cnt[c]))
        self.segs = []                                      # a frame still open closes in a segment yet to come
        return fr, times


def pll_rows(signs: np.ndarray, pllinc: int, state=None):
    """receiver.c:109-135 on one channel's slicer decisions (out > 0), sample by sample: the rows (0-based, within
    `signs`) at which pll > 0xffff after the add at :122-124.  state = (pll, prev), carried; returns (rows, state)."""
    pll, prev = state if state is not None else (0, 0)
    nudge = pllinc // 16
    rows = []
    for i, curr in enumerate(signs.tolist()):
        if curr ^ prev:
            if pll < 0x8000:
                pll += nudge
            else:
                pll -= nudge
        prev = curr
        pll += pllinc
        if pll > 0xffff:
            rows.append(i)
            pll &= 0xffff
    return np.asarray(rows, dtype=np.int64), (pll, prev)


def interp_rows(rows: np.ndarray, n0: int, length: int) -> np.ndarray:
    """the definition's t for every slice of one call [n0, n0 + length), from the true slicing rows (absolute) of it"""
    out = np.empty(len(rows), dtype=np.int64)
    k = 0
    for s in range((length + SEG - 1) // SEG):
        lo = n0 + SEG * s
        l_s = min(SEG, length - SEG * s)
        c_s = int(np.count_nonzero((rows >= lo) & (rows < lo + l_s)))
        for j in range(c_s):
            out[k] = interp(n0, s, j, l_s, c_s)
            k += 1
    assert k == len(rows)
    return out


def time_map(kind: str, n_taps: int = 36, afc_window: int = 0, decim: int = 1, chan_taps: int = 0):
    """gnuais_batch_time_map(): (mul, off), input sample index = t * mul + off"""
    d_f = (n_taps + 1) // 2
    if kind == "audio":
        return 1, -d_f
    if kind == "iq":
        return 1, -d_f - afc_window // 2
    if kind == "wideband":
        return decim, (-d_f - afc_window // 2) * decim + decim - 1 - (chan_taps - 1) // 2
    raise ValueError(kind)
