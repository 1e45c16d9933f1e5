"""NumPy restatement of the wideband channeliser (include/gnuais_hip.h, above gnuais_batch_channeliser) in int64 -- the
yardstick the device's wide stage (wide_kernels.h) is held to bit for bit.  The tables use Python's libm-backed math module, as the
library's host code uses the C library.  Test code only."""
import functools
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


@functools.lru_cache(maxsize=64)
def mixer_table(rate: int, f: int) -> np.ndarray:
    """int16 [P][2] = (C, S), read-only (cached: a period of 2^20 takes a second to tabulate)"""
    P = period(rate, f)
    out = np.empty((P, 2), dtype=np.int16)
    for p in range(P):
        q = (int(f) * p) % int(rate)                     # Python's % is non-negative for a positive modulus
        th = 2.0 * math.pi * float(q) / float(rate)
        out[p, 0] = rnd(32767.0 * math.cos(th))
        out[p, 1] = rnd(32767.0 * math.sin(th))
    out.flags.writeable = False
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
        # polyphase copies: with z zeros in front, ext index a is ph[(a + z) % D][(a + z) // D]
        D, z = self.D, (-(self.T - 1)) % self.D
        ph_r, ph_i = (np.ascontiguousarray(np.concatenate([np.zeros((z,) + v.shape[1:], v.dtype), v])
                                           .reshape((-1, D) + v.shape[1:]).swapaxes(0, 1)) for v in (mr, mi))
        for j in range(self.T):
            h = int(self.h[j])
            if h:
                g, r = divmod(D - 1 + (self.T - 1) - j + z, D)  # row m's sample for tap j: ext index mD + D-1-j + T-1
                acc_r += h * ph_r[r, g:g + rows]
                acc_i += h * ph_i[r, g:g + rows]
        assert np.abs(acc_r).max(initial=0) + 16384 < 2 ** 31 and np.abs(acc_i).max(initial=0) + 16384 < 2 ** 31
        out = np.stack([sat16((acc_r + 16384) >> 15), sat16((acc_i + 16384) >> 15)], axis=-1)
        if self.T > 1:
            self.hist = ext[-(self.T - 1):].copy()
        self.n += L
        return out.reshape(rows, self.M * self.K, 2).astype(np.int16)


def fast_na(K: int, T: int, D: int) -> int:
    """channeliser_fast_na() (resample_plan.cpp): the fast form's accumulators per offset, 0 = the direct form"""
    na = (T + D - 1) // D
    if K < 1 or K > 4:
        return 0
    for b in (4, 8, 17):
        if na <= b:
            return b
    if na <= 33 and K <= 2:
        return 33
    return 0


def ideal(x: np.ndarray, decim: int, rate: int, offsets, taps) -> np.ndarray:
    """The operation the definition approximates, in float64 with no rounding: x int16 [len][M][2], the whole stream
    since reset -> complex128 [len/D][M][K],
        y[m] = (32767/32768) * sum_j h[j] * x[mD + D-1-j] * e^{-j 2 pi ((f n) mod R) / R} / 32768,  n = mD + D-1-j,
    with x = 0 before the first sample.  The angle comes from the exact integer (f n) mod R, not from a table."""
    D, R = int(decim), int(rate)
    x = np.asarray(x)
    L, M = x.shape[0], x.shape[1]
    h = np.asarray(taps, dtype=np.int64)
    T = h.size
    z = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)          # [L][M]
    n = np.arange(L, dtype=np.int64)
    w = np.stack([z * np.exp(-2j * np.pi * (np.mod(int(f) * n, R).astype(np.float64) / R))[:, None]
                  for f in offsets], axis=-1) * (32767.0 / 32768.0)                   # [L][M][K]
    w = np.concatenate([np.zeros((T - 1,) + w.shape[1:], dtype=w.dtype), w])     # index n + T-1
    rows = L // D
    y = np.zeros((rows, M, len(offsets)), dtype=np.complex128)
    for j in range(T):
        if h[j]:
            a = D - 1 + (T - 1) - j
            y += float(h[j]) * w[a:a + (rows - 1) * D + 1:D]
    return y / 32768.0


def torch_channelise(x, decim: int, rate: int, offsets, taps, chunk: int = 512):
    """One call from reset in torch int64 operations, on x's device: x torch int16 [len][M][2] -> torch int16
    [len/D][M*K][2].  The mixer table gathered by n mod P, (u + 16384) >> 15 clamped, then per tap h[j] times a strided
    slice of the mixed values, rounded and clamped -- no code of the library on the path.  Streams in chunks of `chunk`
    to bound memory (about 5 GB at 512 streams of 288 000 samples)."""
    import torch
    D, R = int(decim), int(rate)
    L, M = int(x.shape[0]), int(x.shape[1])
    h = [int(v) for v in np.asarray(taps, dtype=np.int64)]
    T, K, rows = len(h), len(offsets), L // D
    n = torch.arange(L, dtype=torch.int64, device=x.device)
    tabs = []
    for f in offsets:
        tab = torch.from_numpy(mixer_table(R, int(f)).astype(np.int64)).to(x.device)
        p = torch.remainder(n, tab.shape[0])
        tabs.append((tab[p, 0][:, None], tab[p, 1][:, None]))
    out = torch.empty((rows, M, K, 2), dtype=torch.int16, device=x.device)
    for s0 in range(0, M, chunk):
        s1 = min(M, s0 + chunk)
        I = x[:, s0:s1, 0].to(torch.int64)
        Q = x[:, s0:s1, 1].to(torch.int64)
        for k, (Ck, Sk) in enumerate(tabs):
            for c in range(2):
                u = I * Ck + Q * Sk if c == 0 else Q * Ck - I * Sk
                u.add_(16384).bitwise_right_shift_(15).clamp_(-32768, 32767)
                mixed = torch.cat([torch.zeros((T - 1, s1 - s0), dtype=torch.int64, device=x.device), u])
                del u
                acc = torch.zeros((rows, s1 - s0), dtype=torch.int64, device=x.device)
                for j in range(T):
                    if h[j]:
                        a = D - 1 - j + T - 1                  # ext index of row 0's sample for tap j
                        acc.add_(mixed[a:a + (rows - 1) * D + 1:D], alpha=h[j])
                del mixed
                out[:, s0:s1, k, c] = acc.add_(16384).bitwise_right_shift_(15).clamp_(-32768, 32767).to(torch.int16)
                del acc
        del I, Q
    return out.reshape(rows, M * K, 2)
