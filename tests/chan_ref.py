"""NumPy restatement of the wideband channeliser (include/gnuais_hip.h, above gnuais_batch_channeliser) in int64 -- the
yardstick the device's channeliser.hip is held to bit for bit.  The tables use Python's libm-backed math module, as the
library's host code uses the C library.  Test code only."""
import math

import numpy as np


def rnd(x: float) -> int:
    """C lround: round half away from zero, exactly (no x + 0.5 rounding)"""
    a = abs(x)
    f = math.floor(a)
    r = int(f) + (1 if a - f >= 0.5 else 0)
    return -r if x < 0 else r


def period(rate: int, f: int) -> int:
    return rate // math.gcd(abs(int(f)), int(rate))


def mixer_table(rate: int, f: int) -> np.ndarray:
    """int16 [P][2] = (C, S)"""
    P = period(rate, f)
    out = np.empty((P, 2), dtype=np.int16)
    for p in range(P):
        q = (int(f) * p) % int(rate)                     # Python's % is non-negative for a positive modulus
        th = 2.0 * math.pi * float(q) / float(rate)
        out[p, 0] = rnd(32767.0 * math.cos(th))
        out[p, 1] = rnd(32767.0 * math.sin(th))
    return out


def default_taps(decim: int) -> np.ndarray:
    D = int(decim)
    T = 16 * D + 1
    g = []
    for j in range(T):
        w = 0.42 - 0.5 * math.cos(2.0 * math.pi * j / (T - 1)) + 0.08 * math.cos(4.0 * math.pi * j / (T - 1))
        x = 0.75 * (j - 8 * D) / D
        s = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
        g.append(w * s)
    G = 0.0
    for v in g:
        G += v
    return np.array([rnd(v * 32768.0 / G) for v in g], dtype=np.int16)


def sat16(x):
    return np.clip(x, -32768, 32767)


class Channeliser:
    """State of one batch: the configuration, the last T-1 wide samples per stream and n."""

    def __init__(self, M, decim, rate, offsets, taps=None):
        self.M, self.D, self.R = int(M), int(decim), int(rate)
        self.offsets = [int(f) for f in offsets]
        self.K = len(self.offsets)
        self.h = default_taps(decim) if taps is None else np.asarray(taps, dtype=np.int16)
        self.T = int(self.h.size)
        self.tables = [mixer_table(self.R, f).astype(np.int64) for f in self.offsets]
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.T - 1, self.M, 2), dtype=np.int16)
        self.n = 0

    def mix(self, x: np.ndarray, n0: int):
        """x int16 [L][M][2] at wide indices n0 .. -> (mr, mi) int64 [L][M][K]"""
        L = x.shape[0]
        I = x[..., 0].astype(np.int64)[:, :, None]
        Q = x[..., 1].astype(np.int64)[:, :, None]
        n = np.arange(n0, n0 + L, dtype=np.int64)
        C = np.stack([tab[np.mod(n, tab.shape[0]), 0] for tab in self.tables], axis=1)[:, None, :]
        S = np.stack([tab[np.mod(n, tab.shape[0]), 1] for tab in self.tables], axis=1)[:, None, :]
        u = I * C + Q * S
        v = Q * C - I * S
        return sat16((u + 16384) >> 15), sat16((v + 16384) >> 15)

    def run(self, x: np.ndarray) -> np.ndarray:
        """x int16 [len][M][2], len % D == 0 -> int16 [len/D][M*K][2]; advances the state"""
        x = np.asarray(x, dtype=np.int16)
        L = x.shape[0]
        assert x.ndim == 3 and x.shape[1] == self.M and x.shape[2] == 2 and L % self.D == 0
        ext = np.concatenate([self.hist, x], axis=0)     # wide index n - (T-1) ..
        n_first = self.n - (self.T - 1)
        mr, mi = self.mix(ext, n_first)
        if n_first < 0:                                  # before the first sample: mr = 0 (the carry is zero there)
            mr[: -n_first] = 0
            mi[: -n_first] = 0
        rows = L // self.D
        acc_r = np.zeros((rows, self.M, self.K), dtype=np.int64)
        acc_i = np.zeros_like(acc_r)
        e = np.arange(rows) * self.D + self.D - 1 + (self.T - 1)     # ext index of row m's last sample
        for j in range(self.T):
            h = int(self.h[j])
            if h:
                acc_r += h * mr[e - j]
                acc_i += h * mi[e - j]
        assert np.abs(acc_r).max(initial=0) + 16384 < 2 ** 31 and np.abs(acc_i).max(initial=0) + 16384 < 2 ** 31
        out = np.stack([sat16((acc_r + 16384) >> 15), sat16((acc_i + 16384) >> 15)], axis=-1)
        if self.T > 1:
            self.hist = ext[-(self.T - 1):].copy()
        self.n += L
        return out.reshape(rows, self.M * self.K, 2).astype(np.int16)
