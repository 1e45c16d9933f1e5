"""The channeliser's configuration matrix (tests/chan_cases.py) for each sample format that is converted on load (cu8,
cs8, cf32): every fast (K, NA) instance of channeliser_fmt.hip and the direct form for each of its reasons, per format,
with inputs that sit on the formats' edges.  The long k2_na17_P2e20 case stays with cs16: k2_na17_T1025 reaches the same
instance."""
import numpy as np

import chan_cases
from wide_format_ref import DTYPE, VALUE

FORMATS = ("cu8", "cs8", "cf32")
BASE = [c for c in chan_cases.CASES if c.name != "k2_na17_P2e20"]
CASES = [(fmt, c) for fmt in FORMATS for c in BASE]
CASE_IDS = [f"{fmt}-{c.name}" for fmt, c in CASES]


def f32(values):
    return np.array(values, dtype=np.float32)


def neighbours(x):
    """x in fp32 and the fp32 values just below and above it"""
    x = np.float32(x)
    return f32([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


def cf32_specials() -> np.ndarray:
    """+-0, +-1, the largest float below 1, +-inf, NaN of both signs, subnormals, +-1e30; the ties (k + 0.5) / 32768 for
    k = -6 .. 6; the clamp points 32767.5 / 32768 and -32768.5 / 32768 with their fp32 neighbours"""
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff], dtype=np.uint32).view(np.float32)
    sub = np.array([0x00000001, 0x80000001, 0x007fffff, 0x807fffff], dtype=np.uint32).view(np.float32)
    ties = f32([(k + 0.5) / 32768.0 for k in range(-6, 7)])
    return np.concatenate([f32([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), np.inf, -np.inf]),
                           nan, sub, f32([1e30, -1e30]), ties, neighbours(32767.5 / 32768.0),
                           neighbours(-32768.5 / 32768.0)])


def cf32_expected(x: np.ndarray) -> np.ndarray:
    """the definition on fp32 values one by one in Python arithmetic: the fp32 product is exact in a double, round() on
    a float rounds ties to even"""
    out = []
    for v in np.asarray(x, dtype=np.float32):
        y = float(np.float32(v) * np.float32(32768.0)) if np.isfinite(v) else float(v)
        if y != y:
            out.append(0)
        elif y in (float("inf"), float("-inf")):
            out.append(32767 if y > 0 else -32768)
        else:
            out.append(int(min(max(round(y), -32768), 32767)))
    return np.array(out, dtype=np.int16)


def hard_input(rng, n_rows: int, M: int, fmt: str) -> np.ndarray:
    """[n_rows][M][2] in the dtype of fmt.  8-bit: uniform bytes, a quarter of the pairs from 0, 255 (cu8) / -128, 127
    (cs8) and 128 / 0, the codes next to the formats' zero.  cf32: uniform over +-1.1, a quarter of the pairs from
    cf32_specials()."""
    m = rng.random((n_rows, M)) < 0.25
    if fmt == "cf32":
        x = rng.uniform(-1.1, 1.1, (n_rows, M, 2)).astype(np.float32)
        x[m] = rng.choice(cf32_specials(), (int(m.sum()), 2))
        return x
    if fmt == "cu8":
        x = rng.integers(0, 256, (n_rows, M, 2)).astype(np.uint8)
        x[m] = rng.choice(np.array([0, 255, 128, 127], dtype=np.uint8), (int(m.sum()), 2))
        return x
    assert fmt == "cs8", fmt
    x = rng.integers(-128, 128, (n_rows, M, 2)).astype(np.int8)
    x[m] = rng.choice(np.array([-128, 127, 0, -1], dtype=np.int8), (int(m.sum()), 2))
    return x


assert all(DTYPE[f] and VALUE[f] for f in FORMATS)
