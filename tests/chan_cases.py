"""The channeliser's configuration matrix, shared by the CPU tests (tests/test_channeliser_cpu.py) and the device tests
(tests/test_channeliser_forms_gpu.py).  It reaches every channeliser_kernel<K, NA> instance of channeliser.hip and the
direct form for each of its reasons, with T at both edges of a bucket (T = b*D: ceil(T/D) = b, the top of bucket b;
T = b*D + 1: the bottom of the next), D from 1 to 64, odd and even, custom taps (asymmetric, zero at both ends, at the
sum bound 65535), offsets of both signs whose mixer periods differ, and 1 to 4096 streams."""
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

import chan_ref

CALL_ROWS = (1, 37, 300, 2, 129)        # ragged calls, in output rows: 1-row calls are shorter than T-1, 300 rows span
                                        # three 128-row segments


def make_taps(kind: str, T: int, D: int, seed: int) -> np.ndarray:
    """int16 [T] taps of a kind:
    default  the library's design (T must be 16D + 1)
    asym     random magnitudes on a decaying envelope, mostly positive, sum |h| about 40 000 (25 000 at T = 1),
             h != h[::-1]
    zeros    asym with two leading and three trailing zeros
    bound    random signs and magnitudes with sum |h| = 65535 exactly (the largest the definition allows)
    tie      [16384] followed by zeros: acc / 32768 = mr / 2, a rounding tie at every odd mixed value"""
    if kind == "default":
        assert T == 16 * D + 1
        return chan_ref.default_taps(D)
    if kind == "tie":
        h = np.zeros(T, dtype=np.int16)
        h[0] = 16384
        return h
    rng = np.random.default_rng(seed)
    mag = rng.random(T) * np.exp(-2.0 * np.arange(T) / T) + 0.05
    sign = np.where(rng.random(T) < 0.8, 1, -1)
    if kind == "bound":
        assert T >= 3
        mag = np.minimum(mag, 0.45 * mag.sum())                   # no tap may need more than 32767
        h = np.floor(mag * 65535.0 / mag.sum()).astype(np.int64)
        short = 65535 - int(h.sum())
        for i in np.argsort(h)[:short]:                           # short < T; the smallest taps take one more each
            h[i] += 1
        h *= sign
        assert np.abs(h).sum() == 65535 and np.abs(h).max() <= 32767
        return h.astype(np.int16)
    h = np.rint(mag * min(40000.0, 25000.0 * T) / mag.sum()).astype(np.int64) * sign
    if kind == "zeros":
        assert T >= 6
        h[:2] = 0
        h[-3:] = 0
    else:
        assert kind == "asym", kind
    assert np.abs(h).sum() <= 65535 and np.abs(h).max() <= 32767
    if T > 1:
        assert not np.array_equal(h, h[::-1])
    return h.astype(np.int16)


@dataclass(frozen=True)
class Case:
    name: str
    K: int
    D: int
    T: int
    taps_kind: str
    M: int
    R: int
    offsets: Tuple[int, ...]
    na: int                                       # what channeliser_fast_na() picks: the instance, 0 = direct form
    rows: Tuple[int, ...] = CALL_ROWS             # the ragged calls, in output rows

    @property
    def taps(self) -> np.ndarray:
        return make_taps(self.taps_kind, self.T, self.D, seed=self.K * 1000 + self.D * 10 + self.T)

    @property
    def chunks(self) -> List[int]:
        """the calls in wide samples"""
        return [r * self.D for r in self.rows]

    @property
    def direct_reason(self) -> str:
        """why the direct form runs ('' for the fast form)"""
        na = -(-self.T // self.D)
        if self.K > 4:
            return "K>4"
        if na > 33:
            return "ceil(T/D)>33"
        if na > 17 and self.K > 2:
            return "ceil(T/D)>17,K>2"
        return ""


R4 = (-25000, 0, 12345, 125000)            # at 250 kHz: periods 10, 1, 50000, 2
P20 = (1, -262144)                          # at 2^20 Hz: periods 2^20 and 4

CASES = [
    # every (K, NA) instance of the fast form
    Case("k1_na4_T1", 1, 1, 1, "asym", 65, 48000, (12000,), 4),
    Case("k1_na8_bottom", 1, 5, 21, "asym", 63, 240000, (-25000,), 8),
    Case("k1_na17_default", 1, 3, 49, "default", 64, 144000, (25000,), 17),
    Case("k1_na33_bottom", 1, 2, 35, "bound", 1, 96000, (-12345,), 33),
    Case("k2_na4", 2, 8, 25, "zeros", 4096, 384000, (-25000, 25000), 4, rows=(1, 5, 300, 2)),
    Case("k2_na8_top", 2, 7, 56, "asym", 65, 336000, (-25000, 25000), 8),
    Case("k2_na17_P2e20", 2, 16, 257, "default", 1, 1 << 20, P20, 17,
         rows=(1, 37, 3000, 2, 70000, 129, 130000)),                    # 3.25 M wide samples: past 2^20 three times
    Case("k2_na33_top", 2, 3, 99, "zeros", 65, 250000, (12345, 125000), 33),
    Case("k3_na4_top", 3, 64, 256, "asym", 3, 250000, R4[:3], 4),
    Case("k3_na8_top", 3, 5, 40, "bound", 64, 240000, (-25000, 0, 25000), 8),
    Case("k3_na17_bottom", 3, 6, 49, "asym", 65, 288000, (-25000, 0, 25000), 17),
    Case("k3_na17_top", 3, 4, 68, "zeros", 1, 192000, (-25000, 12345, 96000), 17),
    Case("k4_na4_top", 4, 1, 4, "bound", 65, 250000, R4, 4),
    Case("k4_na8", 4, 9, 65, "asym", 63, 250000, R4, 8),
    Case("k4_na17_default", 4, 32, 513, "default", 2, 1536000, (-25000, 25000, -75000, 75000), 17),
    Case("k2_na17_T1025", 2, 64, 1025, "default", 2, 3072000, (-25000, 25000), 17),
    # the direct form, for each of its reasons
    Case("k5_direct", 5, 7, 113, "default", 65, 336000, (-50000, -25000, 0, 25000, 50000), 0),
    Case("k32_direct", 32, 63, 126, "asym", 3, 1008000, tuple(1000 * k - 16000 for k in range(32)), 0),
    Case("k3_na18_direct", 3, 5, 86, "asym", 64, 240000, (-25000, 0, 25000), 0),
    Case("k4_na18_direct", 4, 2, 35, "zeros", 65, 250000, R4, 0),
    Case("k1_na34_direct", 1, 1, 34, "bound", 63, 48000, (-7000,), 0),
]
CASE_IDS = [c.name for c in CASES]


def hard_wide(rng, n_rows: int, M: int) -> np.ndarray:
    """int16 [n_rows][M][2]: uniform, a quarter of the samples at 32767, -32768, -32767 or 0"""
    x = rng.integers(-32768, 32768, (n_rows, M, 2)).astype(np.int16)
    special = np.array([32767, -32768, -32767, 0], dtype=np.int16)
    m = rng.random((n_rows, M)) < 0.25
    x[m] = rng.choice(special, (int(m.sum()), 2))
    return x


def unsaturated_wide(rng, n_rows: int, M: int, taps) -> np.ndarray:
    """int16 [n_rows][M][2] uniform in +-A, A <= 20000 small enough that neither the mix nor the filter saturates:
    |I cos + Q sin| <= sqrt(2) A and |y| <= sum |h| / 32768 * sqrt(2) A <= 30000"""
    s = int(np.abs(np.asarray(taps, dtype=np.int64)).sum())
    A = int(min(20000, 30000 * 32768 / max(s, 1) / 1.415))
    return rng.integers(-A, A + 1, (n_rows, M, 2)).astype(np.int16)


def ideal_bound(taps) -> float:
    """the largest |out - y| per component the definition allows against chan_ref.ideal() where nothing saturates:
    the table's C, S are off by <= 0.5 each, so u = I*C + Q*S is within 0.5 (|I| + |Q|) <= 32768 of 32767 (I cos +
    Q sin): 1.0 after the / 32768; the mix rounds once more, 0.5; so each mixed value is within 1.5 of its ideal.  The
    filter sums sum |h| / 32768 of those errors and rounds once more: 1.5 * sum |h| / 32768 + 0.5 (2.74 for the default
    taps at D = 6)."""
    return 1.5 * float(np.abs(np.asarray(taps, dtype=np.int64)).sum()) / 32768.0 + 0.5


def ideal_errors(out: np.ndarray, y: np.ndarray) -> np.ndarray:
    """out int16 [rows][M*K][2] against y complex128 [rows][M][K] -> float64 errors [rows][M][K][2]"""
    got = out.reshape(y.shape + (2,)).astype(np.float64)
    return np.stack([got[..., 0] - y.real, got[..., 1] - y.imag], axis=-1)
