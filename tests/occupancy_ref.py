"""The channel load per receiver, restated in NumPy int64 from raw I/Q and (frame, time) lists (TEST INFRASTRUCTURE; the
binding definition is in include/gnuais_hip.h under gnuais_batch_occupancy).

  Block j covers the rows [64 j, 64 j + 64); P_j is the int64 sum of I^2 + Q^2 over it.  v0 is the first row of the run of
  I/Q-type calls (or the row the feature was switched on at), b0 = ceil(v0 / 64).
  code(P) = P for P < 8, else 8 (e - 2) + ((P >> (e - 3)) & 7), e = floor(log2 P); power(code) = code for code < 8, else
  (8 + (code & 7)) << (code // 8 - 1).
  Epoch k: the blocks [b0 + k E, b0 + (k + 1) E).  floor = the element of rank E // 8 of its sorted codes; busy_j =
  c_j >= floor + m; bursts counts busy_j and not busy_(j-1), carried from the epoch before, 0 in front of epoch 0;
  cover_j = block j meets the rows [q - S - S_pre, q + S_post] of a frame of the channel whose span begins at or behind v0,
  q = t - d_f - W/2, S = (nbits + 24) 65536 // pllinc, S_pre = 64 * 65536 // pllinc, S_post = 8 * 65536 // pllinc.
  Final once a call of the run ends behind row 64 (b0 + (k + 1) E) - 1 + LAG,
  LAG = (448 + 24) 65536 // pllinc + S_pre + d_f + W/2 + 64.

OccupancyRef is fed the calls as the device is and the frames with their times from anywhere (the device's own drain, or
tests/frame_time_ref.py); epochs() lists every epoch that is final, in the order they became so."""
import numpy as np

B = 64
OCCUPANCY_DTYPE = np.dtype([("floor", "<u2"), ("busy", "<u2"), ("covered", "<u2"), ("bursts", "<u2")])
HELD = 64                                                   # final epochs the library keeps


def code(P):
    """code(P) of the definition for an int or an int64 array, 0 <= P < 2^38 (integer arithmetic only)"""
    P = np.asarray(P, dtype=np.int64)
    e = np.zeros(P.shape, dtype=np.int64)
    for k in range(1, 39):
        e[P >= (np.int64(1) << k)] = k
    big = 8 * (e - 2) + ((P >> np.maximum(e - 3, 0)) & 7)
    out = np.where(P < 8, P, big)
    return int(out) if out.ndim == 0 else out


def power(c):
    """the lower edge of a code's bin"""
    c = np.asarray(c, dtype=np.int64)
    out = np.where(c < 8, c, (8 + (c & 7)) << np.maximum(c // 8 - 1, 0))
    return int(out) if out.ndim == 0 else out


def pre_rows(pllinc: int) -> int:
    return 64 * 65536 // pllinc


def post_rows(pllinc: int) -> int:
    return 8 * 65536 // pllinc


def lag(pllinc: int, n_taps: int = 36, W: int = 0) -> int:
    return (448 + 24) * 65536 // pllinc + pre_rows(pllinc) + (n_taps + 1) // 2 + W // 2 + B


def cover_span(t: int, nbits: int, pllinc: int, n_taps: int = 36, W: int = 0, v0: int = 0):
    """(j_lo, nb): the blocks [j_lo, j_lo + nb) the cover span meets; (0, 0) where the frame covers nothing"""
    if t < 0:
        return 0, 0
    q = t - (n_taps + 1) // 2 - W // 2
    lo = q - (nbits + 24) * 65536 // pllinc - pre_rows(pllinc)
    hi = q + post_rows(pllinc)
    if lo < v0:
        return 0, 0
    return lo // B, hi // B - lo // B + 1


def block_power(iq, n0: int):
    """P_j of the whole blocks inside the rows [n0, n0 + len) of iq [len][n_ch][2]: (first block, int64 [blocks][n_ch])"""
    iq = np.asarray(iq, dtype=np.int16).astype(np.int64)
    P = iq[..., 0] ** 2 + iq[..., 1] ** 2
    j0 = -(-n0 // B)
    j1 = (n0 + len(P)) // B
    if j1 <= j0:
        return j0, np.zeros((0, P.shape[1]), dtype=np.int64)
    return j0, P[j0 * B - n0:j1 * B - n0].reshape(j1 - j0, B, -1).sum(axis=1)


def epoch_record(codes, cover, margin: int, before):
    """one epoch of codes [E][n_ch] and cover [E][n_ch] (bool) with the busy bits `before` [n_ch] in front of it:
    (records [n_ch], tap words [E][n_ch], the busy bits of its last block)"""
    E = codes.shape[0]
    floor = np.sort(codes, axis=0)[E // 8]
    busy = codes >= floor + margin
    prev = np.concatenate([np.asarray(before, dtype=bool)[None], busy[:-1]], axis=0)
    rec = np.zeros(codes.shape[1], dtype=OCCUPANCY_DTYPE)
    rec["floor"] = floor
    rec["busy"] = busy.sum(axis=0)
    rec["covered"] = (busy & cover).sum(axis=0)
    rec["bursts"] = (busy & ~prev).sum(axis=0)
    words = (codes | (busy.astype(np.int64) << 14) | (cover.astype(np.int64) << 15)).astype(np.uint16)
    return rec, words, busy[-1]


class OccupancyRef:
    def __init__(self, n_ch: int, E: int, margin: int, pllinc: int = 0x10000 // 5, n_taps: int = 36, W: int = 0):
        self.n_ch, self.E, self.m = n_ch, E, margin
        self.pllinc, self.n_taps, self.W = pllinc, n_taps, W
        self.reset()

    def reset(self, n: int = 0):
        """the feature is switched on at row n, or the batch is reset: no run yet, nothing final, no frames"""
        self.runs = []                                      # {v0, end, iq: [arrays]}
        self.calls = []                                     # (first row, index of its run or -1 for an audio-type call)
        self.frames = []                                    # (channel, nbits, t)

    def run_iq(self, n0: int, iq):
        iq = np.asarray(iq, dtype=np.int16)
        if not self.runs or self.runs[-1]["end"] != n0:     # the first call, or an audio-type call came between
            self.runs.append({"v0": n0, "end": n0, "iq": []})
        r = self.runs[-1]
        r["iq"].append(iq)
        r["end"] = n0 + len(iq)
        self.calls.append((n0, len(self.runs) - 1))

    def run_audio(self, n0: int, length: int):
        """rows [n0, n0 + length) of an audio-type call: its frames cover nothing, the next I/Q-type call starts a run"""
        self.calls.append((n0, -1))

    def add_frames(self, fr, t):
        for c, nb, tt in zip(fr["channel"], fr["nbits"], t):
            if tt >= 0:
                self.frames.append((int(c), int(nb), int(tt)))

    def epochs(self):
        """[(first block, records [n_ch], tap words [E][n_ch])] of every final epoch, in order"""
        starts = np.array([c[0] for c in self.calls], dtype=np.int64)
        per_run = {}
        for c, nbits, t in self.frames:
            k = int(np.searchsorted(starts, t, side="right")) - 1
            if k >= 0 and self.calls[k][1] >= 0:
                per_run.setdefault(self.calls[k][1], []).append((c, nbits, t))
        out = []
        L = lag(self.pllinc, self.n_taps, self.W)
        for ri, r in enumerate(self.runs):
            b0 = -(-r["v0"] // B)
            n_final = 0
            while r["end"] > B * (b0 + (n_final + 1) * self.E) - 1 + L:
                n_final += 1
            if not n_final:
                continue
            j0, P = block_power(np.concatenate(r["iq"]), r["v0"])
            assert j0 == b0
            codes = code(P[:n_final * self.E])
            cover = np.zeros(codes.shape, dtype=bool)
            for c, nbits, t in per_run.get(ri, []):
                j_lo, nb = cover_span(t, nbits, self.pllinc, self.n_taps, self.W, r["v0"])
                lo, hi = max(j_lo - b0, 0), min(j_lo + nb - b0, len(cover))
                if nb and hi > lo:
                    cover[lo:hi, c] = True
            before = np.zeros(self.n_ch, dtype=bool)
            for k in range(n_final):
                s = slice(k * self.E, (k + 1) * self.E)
                rec, words, before = epoch_record(codes[s], cover[s], self.m, before)
                out.append((b0 + k * self.E, rec, words))
        return out
