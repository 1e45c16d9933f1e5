"""NumPy restatement of the rational U/D channeliser (include/gnuais_hip.h, above gnuais_batch_resampler) in int64 -- the
yardstick the device's resampler.hip is held to bit for bit -- with the float64 operation it approximates (ideal) and a
restatement of the host's plan tables (gnuais_resampler_plan).  The mixer, rnd and sat16 are chan_ref's: the definition
leaves them unchanged.  Test code only."""
import math

import numpy as np

import chan_ref
from chan_ref import rnd, sat16

MAX_UP, MAX_DOWN, MAX_TAPS = 64, 1024, 16385
FAST_NA = 17


def default_taps(up: int, down: int) -> np.ndarray:
    U, D = int(up), int(down)
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
    return np.array([rnd(v * 32768.0 * U / G) for v in g], dtype=np.int16)


def phase_sums(up: int, taps) -> np.ndarray:
    """sum |h[j]| over j = phi (mod U), for each phi"""
    h = np.abs(np.asarray(taps, dtype=np.int64))
    return np.array([h[phi::up].sum() for phi in range(up)], dtype=np.int64)


def check_config(up: int, down: int, taps=None):
    """the definition's limits; ValueError names the one that is broken"""
    if not 1 <= up <= MAX_UP:
        raise ValueError("up range")
    if not 1 <= down <= MAX_DOWN:
        raise ValueError("down range")
    if up >= down:
        raise ValueError("up >= down")
    if math.gcd(up, down) != 1:
        raise ValueError("gcd")
    if taps is not None:
        h = np.asarray(taps, dtype=np.int64)
        if not 1 <= h.size <= MAX_TAPS:
            raise ValueError("tap count")
        if np.abs(h).max() > 32767:
            raise ValueError("tap magnitude")
        if phase_sums(up, h).max() > 65535:
            raise ValueError("phase sum")


def carry_rows(up: int, T: int) -> int:
    return -((-(T - 1)) // up)


def fast_na(K: int, T: int, D: int) -> int:
    """resampler_fast_na() (resample_plan.cpp): one bucket of 17 accumulators per offset for K <= 4, else the direct form"""
    if K < 1 or K > 4:
        return 0
    return FAST_NA if -(-T // D) <= FAST_NA else 0


class Resampler:
    """State of one batch: the configuration, the last H = ceil((T-1)/U) wide samples per stream and n."""

    def __init__(self, M, up, down, rate, offsets, taps=None, max_len=None, check=True):
        """check=False: the arithmetic alone, also where the entry refuses the ratio (U = D = 1 in the tests)"""
        self.M, self.U, self.D, self.R = int(M), int(up), int(down), int(rate)
        self.h = default_taps(up, down) if taps is None else np.asarray(taps, dtype=np.int16)
        if check:
            check_config(self.U, self.D, self.h)
        self.T = int(self.h.size)
        self.H = carry_rows(self.U, self.T)
        self.max_len = max_len
        self.mixer = chan_ref.Channeliser(M, 1, rate, offsets, taps=np.array([1], dtype=np.int16))   # for mix() only
        self.K = self.mixer.K
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.H, self.M, 2), dtype=np.int16)
        self.n = 0

    def run(self, x: np.ndarray) -> np.ndarray:
        """x int16 [len][M][2], len a positive multiple of D -> int16 [len*U/D][M*K][2]; advances the state"""
        x = np.asarray(x, dtype=np.int16)
        L, U, D, T, H = x.shape[0], self.U, self.D, self.T, self.H
        if L <= 0 or L % D:
            raise ValueError("len is not a positive multiple of down")
        rows = L // D * U
        if self.max_len is not None and rows > self.max_len:
            raise ValueError("len * up / down exceeds max_len")
        assert x.ndim == 3 and x.shape[1] == self.M and x.shape[2] == 2 and self.n % D == 0
        ext = np.concatenate([self.hist, x], axis=0)     # wide index n - H ..
        n_first = self.n - H
        mr, mi = self.mixer.mix(ext, n_first)
        if n_first < 0:                                  # before the first sample: mr = 0
            mr[: -n_first] = 0
            mi[: -n_first] = 0
        acc_r = np.zeros((rows, self.M, self.K), dtype=np.int64)
        acc_i = np.zeros_like(acc_r)
        periods = L // D
        # the call starts on a period boundary: local row r = c*U + i ends on local tick e = r*D + D-1 (the call's
        # sample 0 on tick 0), and takes the taps j = e mod U, + U, ... with samples (e - j) / U, one earlier each
        for i in range(U):
            e0 = i * D + D - 1
            j0 = e0 % U
            t0 = (e0 - j0) // U                          # row i's newest sample; row c*U + i: + c*D
            for l, j in enumerate(range(j0, T, U)):
                hj = int(self.h[j])
                if hj:
                    a = H + t0 - l
                    assert a >= 0
                    acc_r[i::U] += hj * mr[a:a + (periods - 1) * D + 1:D]
                    acc_i[i::U] += hj * mi[a:a + (periods - 1) * D + 1:D]
        assert np.abs(acc_r).max(initial=0) + 16384 < 2 ** 31 and np.abs(acc_i).max(initial=0) + 16384 < 2 ** 31
        out = np.stack([sat16((acc_r + 16384) >> 15), sat16((acc_i + 16384) >> 15)], axis=-1)
        if H:
            self.hist = ext[-H:].copy()
        self.n += L
        return out.reshape(rows, self.M * self.K, 2).astype(np.int16)


def ideal(x: np.ndarray, up: int, down: int, rate: int, offsets, taps, tick_shift: int = 0) -> np.ndarray:
    """The operation the definition approximates, in float64 with no rounding, written as what it is: mix (the angle
    from the exact integer (f n) mod R), up-sample by U by zero stuffing, filter with h, keep the ticks m*D + D-1.
    x int16 [len][M][2], the whole stream since reset -> complex128 [len*U/D][M][K].  tick_shift moves the kept ticks
    (tests only: a row one tick late)."""
    U, D, R = int(up), int(down), int(rate)
    x = np.asarray(x)
    L, M = x.shape[0], x.shape[1]
    h = np.asarray(taps, dtype=np.float64)
    T = h.size
    z = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)          # [L][M]
    n = np.arange(L, dtype=np.int64)
    w = np.stack([z * np.exp(-2j * np.pi * (np.mod(int(f) * n, R).astype(np.float64) / R))[:, None]
                  for f in offsets], axis=-1) * (32767.0 / 32768.0)                   # [L][M][K]
    stuffed = np.zeros((L * U + 1,) + w.shape[1:], dtype=np.complex128)           # one more tick for tick_shift
    stuffed[0:L * U:U] = w
    rows = L // D * U
    y = np.zeros((rows,) + w.shape[1:], dtype=np.complex128)
    for m in range(rows):
        u = m * D + D - 1 + tick_shift
        lo = max(0, u - (T - 1))
        seg = stuffed[lo:u + 1][::-1]                    # ticks u, u-1, ..: taps 0, 1, ..
        y[m] = np.tensordot(h[: seg.shape[0]], seg, axes=(0, 0))
    return y / 32768.0


def plan(up: int, down: int, taps):
    """gnuais_resampler_plan() restated: (groups int32 [U][3] = (first, size, base), pairs uint32 [n_pairs][NA], NA, H)"""
    U, D = int(up), int(down)
    h = np.asarray(taps, dtype=np.int64)
    T = h.size
    NA = max(-(-T // D), FAST_NA)                                   # the table's stride: the fast form's bucket at least
    first = [(i * D - 1) // U + 1 for i in range(U + 1)]            # Python's // floors
    groups, base = [], 0
    for i in range(U):
        size = first[i + 1] - first[i]
        groups.append((first[i], size, base))
        base += (size + 1) // 2
    pairs = np.zeros((base, NA), dtype=np.uint32)
    for i, (f, size, b) in enumerate(groups):
        for q in range((size + 1) // 2):
            for a in range(NA):
                v = []
                for k in (f + 2 * q, f + 2 * q + 1):
                    j = (i + a) * D + D - 1 - k * U
                    v.append(int(h[j]) if k < f + size and 0 <= j < T else 0)
                pairs[b + q, a] = (v[0] & 0xffff) | ((v[1] & 0xffff) << 16)
    return np.array(groups, dtype=np.int32), pairs, NA, carry_rows(U, T)


def time_map_ratio(up: int, down: int, chan_taps: int, n_taps: int = 36, afc_window: int = 0):
    """gnuais_batch_time_map_ratio(WIDEBAND): (num, den, off), input sample index = (t * num + off) // den"""
    d_f = (n_taps + 1) // 2
    return down, up, (-d_f - afc_window // 2) * down + down - 1 - (chan_taps - 1) // 2
