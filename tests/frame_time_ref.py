"""The receive time of a frame, restated (TEST INFRASTRUCTURE; the definition is in include/gnuais_hip.h under
gnuais_batch_frame_times).

  n counts the rows the chain has taken since create / reset.  A call that takes rows [n0, n0 + len) is cut into
  segments of 2048 rows; segment s has l_s rows, c_s of which slice.  The bit with index e that closed a frame is the
  j-th slice of some segment s of the call that fed it:   t(e) = n0 + 2048 s + floor((2 j + 1) l_s / (2 c_s)).
  Bits fed without samples (decode_bits) give -1.

The clocks may start anywhere (gnuais_batch_set_clock): FrameTimeRef(rows=R, bits=B) counts n from R and the bits fed on
channel c from B[c], in int64 / Python integers throughout.  The oracle underneath always starts at zero; its records
get their 37-bit stamp (B[c] + stamp) mod 2^37 from shift_frames() and keep the ORACLE's order, which is the order in
time -- a sort of the shifted stamps would hide a device sort on a broken key, and is wrong across the 2^37 wrap.

FrameTimeRef gets c_s from the CPU oracle by feeding it one segment at a time (its state carries across calls, so the
frames are those of the whole call) and applies the formula to the oracle's frames.  pll_rows() is a per-sample
transcription of the reference's loop (src/receiver.c:109-135) that gives the true slicing row of every bit, for the
accuracy test; time_map() restates gnuais_batch_time_map()."""
import numpy as np

from oracle_lib import Oracle

SEG = 2048


def interp(n0: int, s: int, j: int, l_s: int, c_s: int) -> int:
    return n0 + SEG * s + ((2 * j + 1) * l_s) // (2 * c_s)


M37 = (1 << 37) - 1


def stamp(frames: np.ndarray) -> np.ndarray:
    """the 37-bit index of the bit that closed each frame: end_bit and flags[5:1]"""
    return frames["end_bit"].astype(np.int64) | (((frames["flags"].astype(np.int64) >> 1) & 31) << 32)


def shift_frames(frames: np.ndarray, bits) -> np.ndarray:
    """the records of a run that started at zero, as a run that started with bits[channel] bits fed delivers them: the
    37-bit stamp (bits[channel] + stamp) mod 2^37 written back into end_bit and flags bits 5:1; everything else, the
    order included, untouched.  bits: one value per channel, or a scalar."""
    out = frames.copy()
    if len(out) == 0:
        return out
    ch = out["channel"].astype(np.int64)
    b = np.asarray(bits, dtype=np.uint64)
    b = (np.broadcast_to(b, (int(ch.max()) + 1,)) if b.ndim == 0 else b)[ch] & np.uint64(M37)
    e = (b.astype(np.int64) + stamp(out)) & M37
    out["end_bit"] = (e & 0xffffffff).astype(np.uint32)
    out["flags"] = ((out["flags"].astype(np.int64) & ~0x3e) | ((e >> 32) << 1)).astype(np.uint8)
    return out


class FrameTimeRef:
    def __init__(self, n_ch: int, taps=None, pllinc: int = 0, rows: int = 0, bits=None):
        self.o = Oracle(n_ch, taps, pllinc)
        self.n_ch = n_ch
        self.reset(rows, bits)

    def reset(self, rows: int = 0, bits=None):
        """back to the state after create / reset, then set_clock(rows, bits)"""
        self.o.reset()
        self.o.clear_frames()
        self.n = int(rows)                                  # rows taken
        # bits fed per channel: the origin (kept below 2^37, which is all a stamp carries) + what the oracle has seen
        self.bits0 = np.array(np.broadcast_to(np.asarray(0 if bits is None else bits, dtype=np.uint64) & np.uint64(M37),
                                              (self.n_ch,)), dtype=np.int64)
        self.fed = self.bits0.copy()
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
            e = stamp(fr) + self.bits0[fr["channel"].astype(np.int64)]     # not reduced mod 2^37: comparable with `base`
            for i, (c, ei) in enumerate(zip(fr["channel"], e)):
                # the last segment that starts at or before the bit (one without bits shares its start with the next)
                k = int(np.searchsorted(base[:, c], ei, side="right")) - 1
                row0, l_s, b0, cnt = self.segs[k]
                j = int(ei - b0[c])
                assert 0 <= j < cnt[c], (i, c, ei, k)
                times[i] = -1 if row0 < 0 else interp(row0, 0, j, l_s, int(cnt[c]))
        self.segs = []                                      # a frame still open closes in a segment yet to come
        return shift_frames(fr, self.bits0), times


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
