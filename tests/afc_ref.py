"""NumPy restatement of the carrier-error stage (include/gnuais_hip.h, above gnuais_batch_afc): the discriminator of
tests/iq_ref.py, exact int64 block and window sums, and the fp32 phase of a window sum with iq_ref's constants,
operation for operation -- the yardstick the device's afc.hip is held to bit for bit.  Test code only."""
import numpy as np

import iq_ref

B = 64
K = iq_ref.K


def phase(re, im) -> np.ndarray:
    """the header's phase formula from ax = |re| onward: float32 arrays -> int16"""
    f = np.float32
    re, im = np.asarray(re, dtype=f), np.asarray(im, dtype=f)
    with np.errstate(invalid="ignore", divide="ignore"):
        ax, ay = np.abs(re), np.abs(im)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        t = np.where(mx == f(0), f(0), mn / mx).astype(f)
    s = t * t
    p = t * (K["A1"] + s * (K["A3"] + s * (K["A5"] + s * (K["A7"] + s * K["A9"]))))
    p = np.where(ay > ax, K["HALF_PI"] - p, p)
    p = np.where(re < f(0), K["PI"] - p, p)
    p = np.where(im < f(0), -p, p)
    o = np.clip(np.rint(p * K["G"]), f(-32768), f(32767))
    return o.astype(np.int16)


def estimate(SR, SI) -> np.ndarray:
    """e_j of int64 window sums: int64 -> fp32 (round to nearest even), then the phase"""
    return phase(np.asarray(SR, dtype=np.int64).astype(np.float32), np.asarray(SI, dtype=np.int64).astype(np.float32))


def products(iq, prev):
    """r[n], i[n] as exact int64 of pairs iq [len][N][2] after prev [len][N][2]"""
    I, Q = iq[..., 0].astype(np.int64), iq[..., 1].astype(np.int64)
    Ip, Qp = prev[..., 0].astype(np.int64), prev[..., 1].astype(np.int64)
    return I * Ip + Q * Qp, Q * Ip - I * Qp


class Afc:
    """The stage's state for n_ch channels and window W, fed call by call like the device."""

    def __init__(self, n_ch: int, W: int):
        assert W % 128 == 0 and 128 <= W <= 16384
        self.n_ch, self.W, self.L, self.half = n_ch, W, W // 2, W // B // 2
        self.reset()

    def reset(self):
        self.n = 0
        self.carry = None
        self.tail = np.zeros((self.L, self.n_ch), dtype=np.int16)     # a[n - L .. n - 1]
        self.blocks = np.zeros((0, self.n_ch, 2), dtype=np.int64)     # closed blocks, the first one is block self.j0
        self.j0 = 0
        self.open = np.zeros((self.n_ch, 2), dtype=np.int64)          # sums of the rows of block n div 64 so far
        self.last_e = np.zeros(self.n_ch, dtype=np.int16)

    def apply(self, iq) -> np.ndarray:
        """iq int16 [len][n_ch][2] -> the corrected audio int16 [len][n_ch] of these rows"""
        iq = np.asarray(iq, dtype=np.int16)
        ln = iq.shape[0]
        c = np.zeros((self.n_ch, 2), dtype=np.int16) if self.carry is None else self.carry
        prev = np.concatenate([c[None], iq[:-1]], axis=0)
        a, self.carry = iq_ref.discriminate(iq, self.carry)
        r, i = products(iq, prev)
        ri = np.stack([r, i], axis=-1)
        # close the blocks that end inside this call
        n0, n1 = self.n, self.n + ln
        pos = 0
        new = []
        while pos < ln:
            take = min(B - (n0 + pos) % B, ln - pos)
            self.open += ri[pos:pos + take].sum(axis=0)
            pos += take
            if (n0 + pos) % B == 0:
                new.append(self.open.copy())
                self.open[:] = 0
        if new:
            self.blocks = np.concatenate([self.blocks, np.stack(new)], axis=0)
        # the rows' a[m] and e_{m div 64}
        a_ext = np.concatenate([self.tail, a], axis=0)                # row k = a[n0 - L + k]
        out = np.zeros((ln, self.n_ch), dtype=np.int16)
        m = np.arange(n0, n1) - self.L
        ok = m >= 0
        if ok.any():
            j = m[ok] // B
            js = np.arange(j[0], j[-1] + 1)
            cs = np.concatenate([np.zeros((1, self.n_ch, 2), dtype=np.int64), np.cumsum(self.blocks, axis=0)], axis=0)
            lo = np.maximum(js - self.half, 0) - self.j0              # blocks before the stream began count as zero
            hi = js + self.half - self.j0
            assert lo.min() >= 0 and hi.max() <= self.blocks.shape[0], "a block the window needs is not complete"
            S = cs[hi] - cs[lo]
            e = estimate(S[..., 0], S[..., 1])                        # [len(js)][n_ch]
            am = a_ext[:ln][ok].astype(np.int64)
            out[ok] = (am - e[j - j[0]].astype(np.int64)).astype(np.int16)      # two's-complement wrap
            self.last_e = e[-1].copy()
        self.tail = a_ext[ln:]
        self.n = n1
        # blocks older than the oldest window a later call can need
        keep_from = max((self.n - self.L) // B - self.half, 0)
        if keep_from > self.j0:
            self.blocks = self.blocks[keep_from - self.j0:]
            self.j0 = keep_from
        return out

    def estimate(self) -> np.ndarray:
        """e_j of the last output row (0 before there is one)"""
        return self.last_e.copy()


def apply_stream(iq, W: int, cuts=None) -> np.ndarray:
    """the whole stream iq [len][n_ch][2] through a fresh stage, in calls of the given lengths (default: one)"""
    iq = np.asarray(iq, dtype=np.int16)
    st = Afc(iq.shape[1], W)
    if cuts is None:
        return st.apply(iq)
    parts, pos = [], 0
    for n in cuts:
        parts.append(st.apply(iq[pos:pos + n]))
        pos += n
    assert pos == iq.shape[0]
    return np.concatenate(parts, axis=0)
